"""GPU: GT membership in the aggregate verifier's wire readers, and the fast path it opens.  On the tiny job of
tests/test_agg_verify_gpu.py (its helpers, imported): the honest key and proof still deserialise with a context, which now
runs hk_gt_check over every GT member; `verify_aggregate(..., members_in_gt=True)` - Frobenius-split powers for com_lr, z_lr
and TIPP's fold check - gives the default path's verdict and derived values, and every single change of that file's table,
all of which stay inside GT, is rejected with the same reason on both paths; proof bytes whose round message ZL is multiplied
by a cyclotomic element outside GT, or replaced by a canonical random Fq12, and key bytes whose alpha_beta[0] is multiplied by
that element, raise the readers' GT ValueError with a context and still deserialise without one; a point off its curve is
still reported as the point."""
import random

import numpy as np
import pytest

from hekaton_system_amd import agg_verify as av
from hekaton_system_amd.gt import GtField
from hekaton_system_amd.merlin import Transcript as Merlin
from tests import gt_check_cases as gc
from tests.test_agg_verify_gpu import LABEL, _REJECTIONS, _ctx, _read, jobs  # noqa: F401  (jobs: the module's fixture)

pytestmark = pytest.mark.gpu

GT_ERROR = "a GT member is not in the order-r subgroup"


def _rounds_offset(ctx):
    gt = ctx.gt_bytes
    return 8 + 5 * gt + 8 + 4 * (8 + 4 * gt) + 8                       # n, com_ab, com_c, the cross terms, the round count


def _wire_gt(F, data, off):
    return tuple(int.from_bytes(data[off + i * F.nb:off + (i + 1) * F.nb], "little") for i in range(12))


def _with_gt(F, data, off, x):
    out = bytearray(data)
    out[off:off + 12 * F.nb] = F.serialize(x)
    return bytes(out)


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_honest_bytes_deserialize_and_both_paths_agree(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    avk, proof = _read(ctx, cname, j)
    assert avk.serialize() == j.key_bytes and proof.serialize() == j.proof_bytes
    slow, fast = {}, {}
    v_slow = av.verify_aggregate(ctx, avk, j.super_com, j.pub, proof, Merlin(LABEL), trace=slow)
    v_fast = av.verify_aggregate(ctx, avk, j.super_com, j.pub, proof, Merlin(LABEL), trace=fast, members_in_gt=True)
    assert v_slow.ok and v_fast.ok and v_slow.reason == v_fast.reason == av.ACCEPTED
    for key in ("twist", "s", "t", "com_lr", "z_lr"):
        assert slow[key] == fast[key], key
    assert fast["com_lr"] == j.inst["commitment"] and fast["z_lr"] == j.inst["output"]
    # super_com is the caller's own: what the docstring asks the caller to establish, asked of the device
    F = avk.com_h.F
    assert ctx.gt_check(np.frombuffer(F.encode(j.super_com.t) + F.encode(j.super_com.u), np.uint8)).all()


@pytest.mark.parametrize("what", list(_REJECTIONS))
@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_changes_inside_gt_keep_their_reasons_on_both_paths(cname, what, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    change, reason = _REJECTIONS[what]
    for fast in (False, True):
        avk, proof = _read(ctx, cname, j)
        call = dict(super_com=j.super_com, pub=list(j.pub), label=LABEL)
        change(ctx, avk, proof, call)
        F = avk.com_h.F
        members = [proof.com_c.t, proof.com_c.u, call["super_com"].t, call["super_com"].u] + list(avk.alpha_beta) + \
                  [e for row in proof.cross_terms for e in row] + [rd[k] for rd in proof.tipp["rounds"] for k in av._ROUND_KEYS]
        if not fast:                                            # the change stays inside GT: the fast path's premise holds
            assert ctx.gt_check(np.frombuffer(b"".join(F.encode(x) for x in members), np.uint8)).all(), what
        verdict = av.verify_aggregate(ctx, avk, call["super_com"], call["pub"], proof, Merlin(call["label"]), members_in_gt=fast)
        assert not verdict.ok and verdict.reason == reason, (what, fast, verdict)


@pytest.mark.parametrize("kind", ["ZL * c", "random"])
@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_a_round_message_outside_gt_does_not_deserialize(cname, kind, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    F = GtField(cname)
    off = _rounds_offset(ctx) + (1 * 6 + 2) * ctx.gt_bytes                 # round 1, "ZL" is the third of a round's six
    honest = av.AggProof.deserialize(None, cname, j.proof_bytes)
    zl = _wire_gt(F, j.proof_bytes, off)
    assert zl == honest.tipp["rounds"][1]["ZL"]
    if kind == "random":
        rnd = random.Random(5)
        x = tuple(rnd.randrange(F.q) for _ in range(12))
    else:
        x = F.mul(zl, gc.cyclotomic_element(cname))
    assert not F.in_gt(x)
    bad = _with_gt(F, j.proof_bytes, off, x)
    with pytest.raises(ValueError, match="proof: " + GT_ERROR):
        av.AggProof.deserialize(ctx, cname, bad)
    back = av.AggProof.deserialize(None, cname, bad)                       # without a context nothing is checked
    assert back.tipp["rounds"][1]["ZL"] == x and back.serialize() == bad


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_a_key_with_alpha_beta_outside_gt_does_not_deserialize(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    F = GtField(cname)
    honest = av.AggVerifyingKey.deserialize(None, cname, j.key_bytes)
    off = len(j.key_bytes) - len(honest.alpha_beta) * ctx.gt_bytes        # the alpha_beta are the key's last members
    assert _wire_gt(F, j.key_bytes, off) == honest.alpha_beta[0]
    x = F.mul(honest.alpha_beta[0], gc.cyclotomic_element(cname))
    assert not F.in_gt(x)
    bad = _with_gt(F, j.key_bytes, off, x)
    with pytest.raises(ValueError, match="verifying key: " + GT_ERROR):
        av.AggVerifyingKey.deserialize(ctx, cname, bad)
    assert av.AggVerifyingKey.deserialize(None, cname, bad).alpha_beta[0] == x
    # a commitment of the key likewise: com_s[0].t is the first GT member behind the six points and the count
    off_c = 16 + 3 * ctx.g1_bytes + 3 * ctx.g2_bytes + 8
    assert _wire_gt(F, j.key_bytes, off_c) == honest.com_s[0].t
    bad = _with_gt(F, j.key_bytes, off_c, F.mul(honest.com_s[0].t, gc.cyclotomic_element(cname)))
    with pytest.raises(ValueError, match="verifying key: " + GT_ERROR):
        av.AggVerifyingKey.deserialize(ctx, cname, bad)


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_a_point_off_its_curve_is_still_reported_as_the_point(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    F = GtField(cname)
    fq, g1b, g2b = ctx.fq_bytes, ctx.g1_bytes, ctx.g2_bytes
    final_b = _rounds_offset(ctx) + 3 * 6 * ctx.gt_bytes + g1b
    bad = bytearray(j.proof_bytes)
    bad[final_b + 2 * fq if cname == "bn254" else final_b + g2b - 1] ^= 1      # as in tests/test_agg_verify_gpu.py
    with pytest.raises(ValueError, match="G2 point is not on the curve"):
        av.AggProof.deserialize(ctx, cname, bytes(bad))
    # with a GT member outside the subgroup as well, the point check - the earlier one - speaks
    off = _rounds_offset(ctx) + 2 * ctx.gt_bytes
    both = _with_gt(F, bytes(bad), off, F.mul(_wire_gt(F, j.proof_bytes, off), gc.cyclotomic_element(cname)))
    with pytest.raises(ValueError, match="G2 point is not on the curve"):
        av.AggProof.deserialize(ctx, cname, both)
    av.AggProof.deserialize(None, cname, both)
