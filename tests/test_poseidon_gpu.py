"""GPU: hk_poseidon_path (csrc/poseidon.cuh k_poseidon_membership<Fr, 4>, the quad kernel of the job entries, with row b as its
own source and index[b] as its tree index) against hekaton_system_amd/poseidon.py on both curves: the membership block of a
batch of subcircuits - leaf hash, per level (bit, sibling, left), two-to-one hashes - equals
`sha_circuit.poseidon_path_trace` value for value, lands at the requested columns and nowhere else, and its last state
element is the root the host tree computes.  Malformed descriptors / blocks that do not fit are refused.

The seam cases need no tree: the oracle takes arbitrary siblings.  A workgroup holds 64 rows (a quad each), so batch 63 / 64 /
65 are its last quad, a full workgroup and one row into the next, whose other 63 quads recompute that row and store nothing;
depth 0 is the two leaf permutations alone and depth 32 shifts the index by 31.  n_v is the block and five columns."""
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import ExecTree, PoseidonConfig, device_params, merkle_params
from hekaton_system_amd.sha_circuit import poseidon_path_trace

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_membership_block_equals_the_host_trace(cname, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if cname == "bn254" else ctx_bls
    fc = FrCodec(cname)
    r = CURVE_PARAMS[cname]["r"]
    rnd = random.Random(11)
    n = 64                                                     # a 64-leaf execution tree: depth 6, as BASELINE configs[1]
    leaves = [[rnd.randrange(r) for _ in range(4)] for _ in range(n)]
    leaves[5] = [0, 0, 0, 0]
    leaves[6] = [r - 1, 1, r - 1, 0]
    tree = ExecTree(cname, leaves)
    leaf_cfg, node_cfg = merkle_params(cname)
    batch = 70                                                 # more than one wavefront; some leaves twice
    which = [i % n for i in range(batch)]
    traces = [poseidon_path_trace(leaf_cfg, node_cfg, leaves[i], *tree.path(i)) for i in which]
    block = len(traces[0])
    col0, tail = 7, 5
    n_v = col0 + block + tail
    z = capi.DeviceBuffer.from_host(ctx, np.full(batch * n_v * ctx.fr_bytes, 0xA5, np.uint8))
    params = device_params(cname, fc)
    leaf_b = np.stack([fc.enc(leaves[i]) for i in which])
    sib_b = np.stack([fc.enc(tree.path(i)[0]) for i in which])
    idx = np.array(which, np.uint32)
    ctx.poseidon_path(params, leaf_b, sib_b, idx, n_v, col0, z)
    got = z.to_host().reshape(batch, n_v, ctx.fr_bytes)
    for b in range(batch):
        assert fc.dec(got[b, col0:col0 + block].reshape(-1)) == traces[b], (cname, b)
        assert traces[b][-2] == tree.root                      # state[1] of the last permutation
    assert (got[:, :col0] == 0xA5).all() and (got[:, col0 + block:] == 0xA5).all()      # nothing outside the block
    # constants resident on the device give the same result
    cbuf = capi.DeviceBuffer.from_host(ctx, params[0])
    z2 = capi.DeviceBuffer.from_host(ctx, np.zeros(batch * n_v * ctx.fr_bytes, np.uint8))
    ctx.poseidon_path((cbuf,) + params[1:], leaf_b, sib_b, idx, n_v, col0, z2)
    assert np.array_equal(z2.to_host().reshape(batch, n_v, -1)[:, col0:col0 + block], got[:, col0:col0 + block])
    # refused: a block that does not fit, a width the kernel has no state for, constants that end too early
    with pytest.raises(capi.HekatonError) as e:
        ctx.poseidon_path(params, leaf_b, sib_b, idx, n_v - tail - 1, col0, z)
    assert e.value.status == capi.HK_ERR_ARG
    bad = (params[0], params[1], (5,) + params[2][1:], params[3])
    with pytest.raises(capi.HekatonError):
        ctx.poseidon_path(bad, leaf_b, sib_b, idx, n_v, col0, z)
    with pytest.raises(capi.HekatonError):
        ctx.poseidon_path((params[0], params[1] - 4, params[2], params[3]), leaf_b, sib_b, idx, n_v, col0, z)
    for x in (z, z2, cbuf):
        x.free()


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _check_against_trace(ctx, cname, params, cfgs, leaves, sibs, idx):
    """One call over rows of arbitrary leaves / siblings / indices: the block equals the host trace, the 0xA5 around it stays."""
    fc = FrCodec(cname)
    batch, depth = len(leaves), len(sibs[0])
    traces = [poseidon_path_trace(cfgs[0], cfgs[1], leaves[b], sibs[b], idx[b]) for b in range(batch)]
    block = len(traces[0])
    assert block > 0 and all(len(t) == block for t in traces)
    col0, tail = 2, 3
    n_v = col0 + block + tail
    z = capi.DeviceBuffer.from_host(ctx, np.full(batch * n_v * ctx.fr_bytes, 0xA5, np.uint8))
    leaf_b = np.stack([fc.enc(l) for l in leaves])
    sib_b = np.stack([fc.enc(s) for s in sibs]) if depth else np.zeros((batch, 0), np.uint8)
    ctx.poseidon_path(params, leaf_b, sib_b, np.array(idx, np.uint32), n_v, col0, z)
    got = z.to_host().reshape(batch, n_v, ctx.fr_bytes)
    z.free()
    for b in range(batch):
        assert fc.dec(got[b, col0:col0 + block].reshape(-1)) == traces[b], (cname, batch, depth, b)
    assert (got[:, :col0] == 0xA5).all() and (got[:, col0 + block:] == 0xA5).all()


@pytest.mark.parametrize("batch", [1, 63, 64, 65])
@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_batch_seams_of_a_workgroup(cname, batch, ctx_bn254, ctx_bls):
    r = CURVE_PARAMS[cname]["r"]
    rnd = random.Random(1000 + batch)
    leaves = [[rnd.randrange(r) for _ in range(4)] for _ in range(batch)]         # distinct per row
    sibs = [[rnd.randrange(r)] for _ in range(batch)]
    idx = [(7 * b + 3) & 1 for b in range(batch)]                                 # the tree index is not the row
    _check_against_trace(_ctx(cname, ctx_bn254, ctx_bls), cname, device_params(cname, FrCodec(cname)), merkle_params(cname),
                         leaves, sibs, idx)


@pytest.mark.parametrize("depth", [0, 32])
@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_depth_seams(cname, depth, ctx_bn254, ctx_bls):
    r = CURVE_PARAMS[cname]["r"]
    rnd = random.Random(2000 + depth)
    leaves = [[rnd.randrange(r) for _ in range(4)] for _ in range(2)]
    sibs = [[rnd.randrange(r) for _ in range(depth)] for _ in range(2)]
    idx = [0x80000001, 0x7FFFFFFE]                                                # bit 31; both directions at the first and last level
    _check_against_trace(_ctx(cname, ctx_bn254, ctx_bls), cname, device_params(cname, FrCodec(cname)), merkle_params(cname),
                         leaves, sibs, idx)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_zero_round_descriptors(cname, ctx_bn254, ctx_bls):
    """rf = rp = 0, which this entry admits: no round constants, the MDS matrices alone.  A permutation is the identity and
    traces nothing, so the block is (bit, sibling, left) per level with left / right chosen from leaf[0] + leaf[3] upward -
    `poseidon_path_trace` over two zero-round PoseidonConfigs says so itself.  The consts end with the node hash's MDS: the
    kernel's one read past its MDS row, the prefetched first round constant, must stay inside them."""
    fc = FrCodec(cname)
    r = CURVE_PARAMS[cname]["r"]
    cfgs = (PoseidonConfig(r, r.bit_length(), 3, 5, 0, 0), PoseidonConfig(r, r.bit_length(), 2, 17, 0, 0))
    assert cfgs[0].ark == [] and cfgs[1].ark == []
    vals = [v for row in cfgs[0].mds for v in row] + [v for row in cfgs[1].mds for v in row]
    params = (fc.enc(vals), len(vals), (4, 5, 0, 0, 0), (3, 17, 0, 0, 16))
    rnd = random.Random(3000)
    batch, depth = 5, 3
    leaves = [[rnd.randrange(r) for _ in range(4)] for _ in range(batch)]
    sibs = [[rnd.randrange(r) for _ in range(depth)] for _ in range(batch)]
    _check_against_trace(_ctx(cname, ctx_bn254, ctx_bls), cname, params, cfgs, leaves, sibs, [b + 2 for b in range(batch)])
