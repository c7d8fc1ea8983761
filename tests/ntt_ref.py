"""Big-integer reference of the Fr transform layer (csrc/ntt.cuh), one butterfly stage at a time: it knows the stage
arithmetic and the table layouts the kernels document, and nothing of tiles, quads or radix-4 steps.  Plain helper of
tests/test_ntt_ref_cpu.py (which proves it against oracle.pyref.poly) and tests/test_ntt_device_gpu.py.  All values are
plain residues in [0, r); `to_bytes` gives the canonical Montgomery bytes the kernels keep in memory."""
POW_TABLE_BITS = 11
POW_TABLE_SIZE = 1 << POW_TABLE_BITS
FR_BYTES = 32
MONT_R = 1 << 256

_stage_cache = {}


def bitrev_index(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2) if bits else 0


def bitrev(x):
    """the bit-reversal permutation of a vector of 2^k elements"""
    n = len(x)
    bits = n.bit_length() - 1
    assert n == 1 << bits
    return [x[bitrev_index(i, bits)] for i in range(n)]


def root(cp, log_m, inverse):
    w = cp.root_of_unity(log_m)
    return pow(w, -1, cp.r) if inverse else w


def stage_twiddles(cp, s, inverse):
    """w_{2^(s+1)}^j for j < 2^s (w^-1 for inverse)"""
    key = (cp.name, s, bool(inverse))
    if key not in _stage_cache:
        w = root(cp, s + 1, inverse)
        t, acc = [], 1
        for _ in range(1 << s):
            t.append(acc)
            acc = acc * w % cp.r
        _stage_cache[key] = t
    return _stage_cache[key]


def stage_tables(cp, log_table, inverse):
    """the layout documented above k_stage_tables: tws[(2^s - 1) + j] = w_{2^(s+1)}^j, s < log_table, j < 2^s"""
    out = []
    for s in range(log_table):
        out += stage_twiddles(cp, s, inverse)
    assert len(out) == (1 << log_table) - 1
    return out


def squarings(cp, log_table, inverse):
    """sq[k] = w^(2^k), k < log_table, for w the 2^log_table-th root: what NttHost::ensure hands k_pow_table"""
    w = root(cp, log_table, inverse)
    return [pow(w, 1 << k, cp.r) for k in range(log_table)]


def pow_tables(cp, inverse):
    """three levels of POW_TABLE_SIZE entries: g^j, g^(2^11 j), g^(2^22 j) (g^-1 for inverse)"""
    g = pow(cp.fr_generator, -1, cp.r) if inverse else cp.fr_generator
    out = []
    for lvl in range(3):
        b = pow(g, 1 << (POW_TABLE_BITS * lvl), cp.r)
        acc = 1
        for _ in range(POW_TABLE_SIZE):
            out.append(acc)
            acc = acc * b % cp.r
    return out


def pass_ref(cp, x, logn, lo, nst, dit, inverse):
    """stages lo .. lo + nst - 1 of a 2^logn transform, one at a time.  DIF: high to low, (u, v) -> (u + v, (u - v) w);
    DIT: low to high, (u, v) -> (u + v w, u - v w); w = w_{2^(s+1)}^(i mod 2^s) for the pair (i, i + 2^s)."""
    r = cp.r
    n = 1 << logn
    assert len(x) == n and lo + nst <= logn
    a = list(x)
    stages = range(lo, lo + nst) if dit else range(lo + nst - 1, lo - 1, -1)
    for s in stages:
        tw = stage_twiddles(cp, s, inverse)
        span = 1 << s
        for blk in range(0, n, 2 * span):
            us, vs = a[blk:blk + span], a[blk + span:blk + 2 * span]
            if dit:
                vs = [v * w % r for v, w in zip(vs, tw)]
                a[blk:blk + span] = [(u + v) % r for u, v in zip(us, vs)]
                a[blk + span:blk + 2 * span] = [(u - v) % r for u, v in zip(us, vs)]
            else:
                a[blk:blk + span] = [(u + v) % r for u, v in zip(us, vs)]
                a[blk + span:blk + 2 * span] = [(u - v) * w % r for u, v, w in zip(us, vs, tw)]
    return a


def epilogue_ref(cp, x, logn, post, scale, g, sub, kc):
    """the fused epilogue of k_ntt_pass4 in its documented order: post & 2 -> x[i] *= g^bitrev(i); post & 4 ->
    x[i] -= sub[i] * kc; post & 1 -> x[i] *= scale"""
    r = cp.r
    out = []
    for i, v in enumerate(x):
        if post & 2:
            v = v * pow(g, bitrev_index(i, logn), r) % r
        if post & 4:
            v = (v - sub[i] * kc) % r
        if post & 1:
            v = v * scale % r
        out.append(v)
    return out


def to_bytes(cp, xs):
    """plain residues -> canonical Montgomery bytes, 32 per element, little-endian"""
    return b"".join((x * MONT_R % cp.r).to_bytes(FR_BYTES, "little") for x in xs)
