"""CPU: the prove-lane stream plan (hekaton_system_amd/csrc/stream_plan.h).  A context's
PROVE_COALESCE_RUNNING prove lanes get s = clamp(Q / K, 1, 5) streams each out of the Q hardware queues, and a chunk's five
roles (main, B1, B2, L, H) fold onto those s streams by a fixed table."""
import subprocess

import pytest

from tests import host_build

ROLES = ("main", "B1", "B2", "L", "H")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_driver")
    host_build.build("stream_plan_driver.cpp", exe, "-O1", "-Wall", "-Werror")
    s, maps = {}, {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if f[0] == "s":
            s[int(f[1]), int(f[2])] = int(f[3])
        else:
            maps[int(f[1])] = dict(zip(ROLES, map(int, f[2:])))
    return s, maps


def test_streams_per_lane(plan):
    s, _ = plan
    assert s[4, 2] == 2 and s[20, 2] == 5 and s[8, 2] == 4 and s[6, 2] == 3
    assert s[1, 2] == 1 and s[0, 2] == 1 and s[40, 2] == 5 and s[3, 2] == 1
    for (q, k), v in s.items():
        assert v == min(max(q // k, 1), 5)
        # the prove lanes never ask for more streams than there are queues, unless one stream per lane is already more
        assert v * k <= q or v == 1


def test_role_map(plan):
    _, maps = plan
    groups = {}
    for n, m in maps.items():
        assert m["main"] == 0
        assert sorted(set(m.values())) == list(range(n)), "every stream of the lane carries a role"
        g = {}
        for role, st in m.items():
            g.setdefault(st, set()).add(role)
        groups[n] = sorted(frozenset(v) for v in g.values())
    want = {1: [{"main", "B1", "B2", "L", "H"}],
            2: [{"main", "B1", "B2", "L"}, {"H"}],
            3: [{"main", "L"}, {"B1", "B2"}, {"H"}],
            4: [{"main", "L"}, {"B1"}, {"B2"}, {"H"}],
            5: [{r} for r in ROLES]}
    for n, w in want.items():
        assert groups[n] == sorted(frozenset(x) for x in w), n
    # from two streams on, H never shares a stream with the other roles
    for n in range(2, 6):
        assert list(maps[n].values()).count(maps[n]["H"]) == 1
