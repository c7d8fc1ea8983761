"""CPU: hk_vkd_tree's host side - the declaration and its binding, the host mirror
`vkd_circuit.directory_paths` against the paths the fixtures built by hand, the restated level recurrence of
tests/vkd_tree_cases.py (what the kernels run) against that mirror, and the errors of `VkdJob(siblings=...)`."""
import os
import re

import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.vkd_circuit import Append, Update, VkdJob, concat, directory_paths
from tests import vkd_tree_cases as vc
from tests.vkd_fixtures import DEPTH, SPLIT, updates_b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    assert re.search(r"hk_status\s+hk_vkd_tree\s*\(\s*hk_ctx\s*\*\s*ctx,\s*const\s+hk_vkd_tree_desc\s*\*", header)
    for st, v in (("OK", 0), ("OCCUPIED", 1), ("ABSENT", 2), ("STALE", 3)):
        assert re.search(r"#define\s+HK_VKD_ST_%s\s+%du" % (st, v), header)
    assert "hk_vkd_tree" in capi.EXPORTS
    fields = [f for f, _ in capi.hk_vkd_tree_desc._fields_]
    body = re.search(r"typedef struct \{([^}]*)\}\s*hk_vkd_tree_desc;", header).group(1)
    declared = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == declared
    core = open(os.path.join(ROOT, "hekaton_system_amd", "csrc", "hk_core.hip")).read()
    assert "ctx->ops->vkd_tree(" in core


@pytest.mark.parametrize("curve", vc.CURVES)
def test_mirror_reproduces_fixture_b(curve):
    genesis = concat(bytes(32), bytes(32), 0)
    initial, final, ups = updates_b(curve)
    got = directory_paths(curve, DEPTH, [genesis], ups)
    assert got == (initial, final, [u.path for u in ups], [0, 0, 0])


@pytest.mark.parametrize("curve", vc.CURVES)
def test_mirror_reproduces_random_job(curve):
    job = VkdJob.random(curve, 5, 32, 4)
    genesis = concat(bytes(32), bytes(32), 0)
    got = directory_paths(curve, 32, [genesis], job.updates)
    assert got == (job.initial_root, job.final_root, [u.path for u in job.updates], [0] * len(job.updates))


@pytest.mark.parametrize("which", vc.SMALL_CASES)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_recurrence_equals_mirror(curve, which):
    depth, leaves0, changes = vc.case(curve, which)
    initial, final, paths, _ = vc.mirror(curve, which)
    events = vc.events_of(curve, depth, leaves0, changes)
    sibs, root0, root1, order = vc.recurrence(curve, depth, events, len(leaves0))
    assert sibs == paths
    assert (root0, root1) == (initial, final)
    assert order == list(range(len(events)))


def test_threshold_is_straddled():
    src = open(os.path.join(ROOT, "hekaton_system_amd", "csrc", "vkd_tree.cuh")).read()
    assert int(re.search(r"VT_WG_EVENTS\s*=\s*(\d+)", src).group(1)) == vc.WG_EVENTS
    sizes = sorted(len(vc.case("bn254", w)[1]) + len(vc.case("bn254", w)[2]) for w in ("g63", "g64", "g65"))
    assert sizes == [vc.WG_EVENTS - 1, vc.WG_EVENTS, vc.WG_EVENTS + 1]


class _FakeBuffer(capi.DeviceBuffer):
    def __init__(self, nbytes):                        # noqa: no allocation: the checks read the size only
        self.ctx, self.ptr, self.nbytes = None, 0, nbytes


def test_job_siblings_errors():
    curve = "bn254"
    initial, final, ups = updates_b(curve)
    bare = [Append(u.username, u.key) if isinstance(u, Append) else Update(u.username, u.counter, u.key1, u.key2) for u in ups]
    assert all(u.path is None for u in bare)
    good = _FakeBuffer(len(ups) * DEPTH * 32)
    with pytest.raises(ValueError):                    # device siblings, host values
        VkdJob(curve, initial, final, bare, depth=DEPTH, split=SPLIT, siblings=good)
    with pytest.raises(ValueError):                    # another size than U x depth Fr
        VkdJob(curve, initial, final, bare, depth=DEPTH, split=SPLIT, host_values=False, siblings=_FakeBuffer(good.nbytes - 32))
    with pytest.raises(ValueError):                    # no DeviceBuffer
        VkdJob(curve, initial, final, bare, depth=DEPTH, split=SPLIT, host_values=False, siblings=bytes(good.nbytes))
    with pytest.raises(ValueError):                    # no path and no siblings
        VkdJob(curve, initial, final, bare, depth=DEPTH, split=SPLIT)
    job = VkdJob(curve, initial, final, bare, depth=DEPTH, split=SPLIT, host_values=False, siblings=good)
    assert job.tables()["siblings"] is good and job.values is None
    host = VkdJob(curve, initial, final, ups, depth=DEPTH, split=SPLIT)
    assert (job.slot_addr == host.slot_addr).all() and (job.slot_src == host.slot_src).all()
