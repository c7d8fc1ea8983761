"""TIPP: the inner-pairing-product argument the aggregator finishes with (`TIPA::prove / verify`,
distributed-prover/src/aggregation.rs:337-340), host orchestration over the GPU primitives.

The reference takes `TIPA` from the third-party `ripp` crate (`ark_ip_proofs::tipa`, branch ip-commitment-old, absent
from /root/reference) with the SnarkPack commitment (`ip_commitment::snarkpack::TIPPCommitment`) and keeps its own copy
of the KZG half in distributed-prover/src/kzg.rs (`KzgComKey::gen`, `prove_commitment_v/w`, `prove_evaluation`: :46-155).
This module restates the protocol from that file and from the SnarkPack paper (Gailly, Maller, Nitulescu, section 5:
GIPA with the pair commitment, rescaled w-key for the twist, KZG openings of the final keys) - PARITY UNPINNED: the
Fiat-Shamir transcript here is plain SHA-256 over the canonical encodings (the reference uses merlin through ripp's
`ProtoTranscript`), so challenges, and therefore proof bytes, are this build's own.  What the tests pin
(tests/test_tipa_gpu.py): completeness on real aggregation instances, soundness smoke tests (any tampered element,
commitment, output or twist is rejected), the folded keys against the closed-form `ipa_polynomial`, and the KZG
identities.

Statement:  (T, U) = commit_with_ip(ck, A, B)  and  Z = prod_i e(A_i, B_i)^(r^i)   (`twisted_inner_product`).
    ck: v1 = h^(a^i), v2 = h^(b^i), w1 = g^(a^(n+i)), w2 = g^(b^(n+i));  T = A*v1 . w1*B,  U = A*v2 . w2*B.
Prover: B' = B^(r^i), w' = w^(r^-i) (so the commitment of (A, B') under (v, w') is the given one), then log n rounds:
    cross commitments L = pair(v_L, w'_R; A_R, B'_L), R = pair(v_R, w'_L; A_L, B'_R) and cross products,
    challenge c, fold A <- A_L + c A_R, B' <- B'_L + c^-1 B'_R, v <- v_L + c^-1 v_R, w' <- w'_L + c w'_R;
    finally KZG openings of the folded keys at a random point against
        f_v(X) = prod_k (1 + c_(l-1-k)^-1 X^(2^k)),     f_w(X) = X^n prod_k (1 + c_(l-1-k) (X / r)^(2^k)).
GPU work per round: 10 multi-pairings of n/2 pairs (two hk_pairing_products calls), 6 element-wise folds
(hk_points_lincomb); at the end four MSMs over the resident SRS (hk_msm_bases).  The scalar vectors - the trapdoor powers
of `setup`, the twist powers and the two KZG quotients of `prove` - are built on the device too (hk_scalar_powers,
hk_ipa_quotient) and read where they lie; HK_AGG_HOST_SCALARS=1 in the environment keeps the Python loops.
"""
import hashlib
import os
import time
from concurrent.futures import ThreadPoolExecutor, wait
from dataclasses import dataclass, field

import numpy as np

from .aggregation import IPCommKey, TIPPCommitment, host_scalars
from .cp_groth16 import CURVE_PARAMS, FrCodec
from .gt import GtField


@dataclass
class Srs:
    """`KzgComKey` (kzg.rs:30-43) + the commitment key derived from it.  g_alpha / g_beta: 2n G1 powers; h_alpha / h_beta:
    n G2 powers (resident on the device for the opening MSMs)."""
    n: int
    g_alpha: np.ndarray
    g_beta: np.ndarray
    h_alpha: np.ndarray
    h_beta: np.ndarray
    ck: IPCommKey
    resident: dict = field(default_factory=dict)


def setup(ctx, curve, n, alpha, beta):
    """`KzgComKey::gen` (kzg.rs:72-119) with caller-supplied trapdoors; n a power of two."""
    assert n >= 2 and n & (n - 1) == 0
    p = CURVE_PARAMS[curve]
    fc = FrCodec(curve)
    r = p["r"]
    G1, G2 = fc.g1(p["g1"]), fc.g2(p["g2"])
    fr = ctx.fr_bytes
    scalars = None
    if host_scalars():
        pa, pb = [fc.R % r] * (2 * n), [fc.R % r] * (2 * n)          # R * alpha^i: Montgomery values as they come
        for i in range(1, 2 * n):
            pa[i] = pa[i - 1] * alpha % r
            pb[i] = pb[i - 1] * beta % r
        sc1, sc2 = fc.enc_canon(pa + pb), fc.enc_canon(pa[:n] + pb[:n])
    else:
        # alpha^i | beta^i, 2 n each for G1 and n each for G2, written where the two sweeps read them
        from .capi import DeviceBuffer
        scalars = DeviceBuffer(ctx, 6 * n * fr)
        sc1, sc2 = scalars.view(0, 4 * n * fr), scalars.view(4 * n * fr, 2 * n * fr)
    try:
        return _setup(ctx, n, alpha, beta, G1, G2, sc1, sc2)
    finally:
        if scalars is not None:                                       # every call that read it has returned
            scalars.free()


def _setup(ctx, n, alpha, beta, G1, G2, sc1, sc2):
    fr = ctx.fr_bytes
    if not isinstance(sc1, np.ndarray):
        for buf, m, x, off in ((sc1, 2 * n, alpha, 0), (sc1, 2 * n, beta, 2 * n), (sc2, n, alpha, 0), (sc2, n, beta, n)):
            ctx.scalar_powers(x, m, 1, buf.view(off * fr, m * fr))
    # two fixed-base sweeps (one per generator: its window table is built once, or comes from the context's cache), then
    # four uploads: issued together (one lane each)
    with ThreadPoolExecutor(max_workers=4) as pool:
        f1 = pool.submit(ctx.fixed_base, 1, G1, sc1, 4 * n)
        f2 = pool.submit(ctx.fixed_base, 2, G2, sc2, 2 * n)
        g1b, g2b = ctx.g1_bytes, ctx.g2_bytes
        g_ab, h_ab = np.asarray(f1.result()), np.asarray(f2.result())
        g_a, g_b = g_ab[:2 * n * g1b], g_ab[2 * n * g1b:]
        h_a, h_b = h_ab[:n * g2b], h_ab[n * g2b:]
        ck = IPCommKey(v1=h_a, v2=h_b, w1=g_a[n * g1b:].copy(), w2=g_b[n * g1b:].copy(), n=n)
        srs = Srs(n, g_a, g_b, h_a, h_b, ck)
        ups = [pool.submit(ctx.bases_upload, g, v) for g, v in ((1, g_a), (1, g_b), (2, h_a), (2, h_b))]
        srs.resident = dict(zip(("g_alpha", "g_beta", "h_alpha", "h_beta"), (f.result() for f in ups)))
    return srs


class Transcript:
    """SHA-256 chaining (NOT the reference's merlin transcript): state <- H(state || label || data)."""

    def __init__(self, r_mod, label=b"hekaton-tipp"):
        self.state = hashlib.sha256(label).digest()
        self.r = r_mod

    def absorb(self, label, *chunks):
        h = hashlib.sha256(self.state + label)
        for c in chunks:
            h.update(bytes(c))
        self.state = h.digest()

    def challenge(self, label):
        ctr = 0
        while True:
            d = hashlib.sha256(self.state + label + bytes([ctr])).digest() + hashlib.sha256(self.state + label + bytes([ctr, 1])).digest()
            v = int.from_bytes(d, "little") % self.r
            if v:
                self.state = hashlib.sha256(self.state + d).digest()
                return v
            ctr += 1


def ipa_polynomial_coeffs(challenges, r_shift, mod, scale=1):
    """pairing_ops.rs `ipa_polynomial`: coefficients of prod_k (1 + challenges[k] (r_shift X)^(2^k)), degree 2^l - 1, times
    `scale` (the Montgomery constant R: quotients of a scaled polynomial come out in Montgomery form with no further
    product per coefficient)."""
    coeffs = [scale % mod]
    power = r_shift % mod
    for c in challenges:
        factor = c * power % mod
        coeffs = coeffs + [x * factor % mod for x in coeffs]
        power = power * power % mod
    return coeffs


def ipa_polynomial_eval(challenges, r_shift, z, mod):
    out, power = 1, r_shift * z % mod
    for c in challenges:
        out = out * (1 + c * power) % mod
        power = power * power % mod
    return out


def _divide_by_linear(coeffs, z, mod):
    """Quotient of the polynomial by (X - z) (ark `&poly / &(X - z)`: the remainder f(z) is dropped)."""
    n = len(coeffs)
    q = [0] * n
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (coeffs[i] + acc * z) % mod
        q[i - 1] = acc
    return q                      # q[n-1] = 0: same length as the SRS slice, as kzg.rs:133-135 resizes it


def twist_vectors(ctx, fc, twist, twist_inv, n, out=None):
    """(twist^i, twist^-i), i < n, as Montgomery bytes: what `prove` sweeps B and the w-keys with.  On the device
    (hk_scalar_powers) into the two windows `out` of n Fr each, which are returned; under HK_AGG_HOST_SCALARS the Python
    loop's host bytes.  The two calls go out one after the other: each is shorter than a hand-over to the pool."""
    if host_scalars():
        r = fc.r
        vecs = []
        for x in (twist, twist_inv):
            pw = [fc.R % r] * n                   # R * x^i: the Montgomery bytes with no product beyond the power itself
            for i in range(1, n):
                pw[i] = pw[i - 1] * x % r
            vecs.append(fc.enc_canon(pw))
        return tuple(vecs)
    ctx.scalar_powers(twist, n, 1, out[0])
    ctx.scalar_powers(twist_inv, n, 1, out[1])
    return tuple(out)


def opening_quotients(ctx, fc, challenges, twist_inv, z, n, out=None):
    """The KZG witness polynomials of the folded keys (kzg.rs:122-141) as Montgomery bytes: q_v = f_v / (X - z) (n Fr) and
    q_w = f_w / (X - z) (2 n Fr), from the rounds' challenges in the order they were drawn.  On the device (hk_ipa_quotient)
    into the two windows `out`, which are returned; under HK_AGG_HOST_SCALARS the Python loops' host bytes."""
    r = fc.r
    ch_rev = challenges[::-1]
    chi_rev = [pow(c, -1, r) for c in ch_rev]
    if host_scalars():
        fv = ipa_polynomial_coeffs(chi_rev, 1, r, fc.R)                    # R f(X): the quotients are Montgomery values
        fw = [0] * n + ipa_polynomial_coeffs(ch_rev, twist_inv, r, fc.R)
        return fc.enc_canon(_divide_by_linear(fv, z, r)), fc.enc_canon(_divide_by_linear(fw, z, r))
    ctx.ipa_quotient(chi_rev, 1, z, 0, out[0])
    ctx.ipa_quotient(ch_rev, twist_inv, z, n, out[1])
    return tuple(out)


# vectors of the recursion, by their index in the arena: G1 vectors fold with the challenge c, G2 vectors with 1 / c
_A, _B, _V1, _V2, _W1, _W2 = range(6)
_G1_VECS, _G2_VECS = (_A, _W1, _W2), (_B, _V1, _V2)
# a round's messages as inner products <X, Y> between a G1 vector X and a G2 vector Y: T over (a, v1) and (w1, b), U over
# (a, v2) and (w2, b), Z over (a, b); the L message pairs X's right half with Y's left half, the R message the reverse
_NAME_PAIRS = ((_A, _V1), (_W1, _B), (_A, _V2), (_W2, _B), (_A, _B))
_MESSAGES = (("T", (0, 1)), ("U", (2, 3)), ("Z", (4,)))
# quarter-by-quarter inner products E[i][j] = <X_i, Y_j> a pair of rounds needs (X = X_0 | X_1 | X_2 | X_3):
#   round k      L: <X_R, Y_L> = E[2][0] E[3][1]                           R: <X_L, Y_R> = E[0][2] E[1][3]
#   round k + 1  on X' = X_L + c X_R, Y' = Y_L + Y_R / c (bilinearity):
#                L: <X'_R, Y'_L> = E[1][0] E[1][2]^(1/c) E[3][0]^c E[3][2]    R: <X'_L, Y'_R> = E[0][1] E[0][3]^(1/c) E[2][1]^c E[2][3]
_QUARTERS = ((2, 0), (3, 1), (0, 2), (1, 3), (1, 0), (1, 2), (3, 0), (3, 2), (0, 1), (0, 3), (2, 1), (2, 3))
_Q = {ij: t for t, ij in enumerate(_QUARTERS)}


def _fold(ctx, go, win, pos, m, c, c_inv):
    """The six vectors of size m at `pos` folded to size m / 2 right behind them; returns the new position."""
    h, nxt = m // 2, pos + m
    L = lambda k: win(k, pos, h)
    R = lambda k: win(k, pos + h, h)
    # the three G1 folds share c, the three G2 folds 1 / c: one batched call per group, issued together (the G2 fold is
    # the longer one: it goes out from this thread, the G1 fold beside it from the pool)
    g1_fold = go(ctx.points_fold_many, 1, [L(k) for k in _G1_VECS], [R(k) for k in _G1_VECS], c, h, [win(k, nxt, h) for k in _G1_VECS])
    ctx.points_fold_many(2, [L(k) for k in _G2_VECS], [R(k) for k in _G2_VECS], c_inv, h, [win(k, nxt, h) for k in _G2_VECS])
    g1_fold.result()
    return nxt


def _single_round(ctx, F, r, win, pos, m, tr, go, rounds, challenges, times):
    h = m // 2
    L = lambda k: win(k, pos, h)
    R = lambda k: win(k, pos + h, h)
    # all ten multi-pairings of the round in ONE batched call: ten (lhs, rhs) pairs out of 6 x 6, every G2 vector's Miller
    # lines computed once
    t0 = time.perf_counter()
    pp = ctx.pairing_pairs([R(_A), L(_A), R(_W1), R(_W2), L(_W1), L(_W2)], [L(_V1), L(_V2), L(_B), R(_V1), R(_V2), R(_B)],
                           [(0, 0), (2, 2), (0, 1), (3, 2), (0, 2), (1, 3), (4, 5), (1, 4), (5, 5), (1, 5)], h)
    t1 = time.perf_counter()
    D = F.decode
    TL = F.mul(D(pp[0]), D(pp[1])); UL = F.mul(D(pp[2]), D(pp[3])); ZL = D(pp[4])
    TR = F.mul(D(pp[5]), D(pp[6])); UR = F.mul(D(pp[7]), D(pp[8])); ZR = D(pp[9])
    tr.absorb(b"round", *(F.encode(x) for x in (TL, UL, ZL, TR, UR, ZR)))
    c = tr.challenge(b"c")
    rounds.append(dict(TL=TL, UL=UL, ZL=ZL, TR=TR, UR=UR, ZR=ZR))
    challenges.append(c)
    t2 = time.perf_counter()
    nxt = _fold(ctx, go, win, pos, m, c, pow(c, -1, r))
    times.append((m, t1 - t0, t2 - t1, time.perf_counter() - t2))
    return nxt


def _round_pair(ctx, F, fc, r, win, pos, m, tr, go, rounds, challenges, times):
    """Two rounds for one pass through the pairing pipeline: the messages of round k + 1 are inner products of the FOLDED
    vectors, and by bilinearity those are products of quarter-by-quarter inner products of the current vectors raised to
    1, c, 1 / c - so the sixty quarter products both rounds need are taken in ONE batched call (one lines / tree / Horner
    chain instead of two), round k's messages are products of them, and round k + 1's one grouped multi-exponentiation
    that runs beside round k's fold.  The messages are the same GT elements, bit for bit, as round by round."""
    q = m // 4
    t0 = time.perf_counter()
    quarter = lambda k, i: win(k, pos + i * q, q)
    lhs = [quarter(k, i) for k in _G1_VECS for i in range(4)]
    rhs = [quarter(k, j) for k in _G2_VECS for j in range(4)]
    pairs = [(4 * _G1_VECS.index(x) + i, 4 * _G2_VECS.index(y) + j) for x, y in _NAME_PAIRS for i, j in _QUARTERS]
    E = np.asarray(ctx.pairing_pairs(lhs, rhs, pairs, q), np.uint8).reshape(len(pairs), -1)
    t1 = time.perf_counter()
    e = lambda p, i, j: E[len(_QUARTERS) * p + _Q[(i, j)]]
    one = np.frombuffer(F.encode(F.one), np.uint8)

    def messages(factors_of, c, c_inv):
        """(TL, UL, ZL, TR, UR, ZR) as ONE grouped multi-exponentiation: factors_of(side) lists ((i, j), exponent) per name pair."""
        bases, exps = [], []
        for side in "LR":
            for _name, members in _MESSAGES:
                for p in members:
                    for (i, j), k in factors_of(side, c, c_inv):
                        bases.append(e(p, i, j)); exps.append(k)
                for _pad in range((2 - len(members)) * len(factors_of(side, c, c_inv))):
                    bases.append(one); exps.append(0)
        glen = len(bases) // 6
        out = ctx.gt_pow_prod(np.concatenate(bases), fc.enc(exps), glen)
        return [F.decode(out[g]) for g in range(6)]

    def absorb(msgs):
        TL, UL, ZL, TR, UR, ZR = msgs
        tr.absorb(b"round", *(F.encode(x) for x in msgs))
        c = tr.challenge(b"c")
        rounds.append(dict(TL=TL, UL=UL, ZL=ZL, TR=TR, UR=UR, ZR=ZR))
        challenges.append(c)
        return c, pow(c, -1, r)

    now = lambda side, c, ci: ((((2, 0), 1), ((3, 1), 1)) if side == "L" else (((0, 2), 1), ((1, 3), 1)))
    nxt_round = lambda side, c, ci: ((((1, 0), 1), ((1, 2), ci), ((3, 0), c), ((3, 2), 1)) if side == "L" else
                                     (((0, 1), 1), ((0, 3), ci), ((2, 1), c), ((2, 3), 1)))
    c, c_inv = absorb(messages(now, 1, 1))
    t2 = time.perf_counter()
    f_next = go(messages, nxt_round, c, c_inv)                    # round k + 1's messages, beside round k's fold
    pos1 = _fold(ctx, go, win, pos, m, c, c_inv)
    t3 = time.perf_counter()
    c2, c2_inv = absorb(f_next.result())
    t4 = time.perf_counter()
    pos2 = _fold(ctx, go, win, pos1, m // 2, c2, c2_inv)
    times.append((m, t1 - t0, t2 - t1, t3 - t2))
    times.append((m // 2, 0.0, t4 - t3, time.perf_counter() - t4))
    return pos2


def gipa_rounds(ctx, F, fc, r, win, n, tr, go, rounds, challenges, times, paired=True):
    """The log2(n) rounds of the recursion over the six device-resident vectors `win(k, start, count)` addresses; appends
    the rounds' messages and challenges, returns the position of the final single elements."""
    m, pos = n, 0
    while m > 1:
        if paired and m >= 4:
            pos = _round_pair(ctx, F, fc, r, win, pos, m, tr, go, rounds, challenges, times)
            m //= 4
        else:
            pos = _single_round(ctx, F, r, win, pos, m, tr, go, rounds, challenges, times)
            m //= 2
    return pos


class Tipp:
    def __init__(self, ctx, curve):
        self.ctx, self.curve = ctx, curve
        self.fc = FrCodec(curve)
        self.F = GtField(curve)
        self.r = CURVE_PARAMS[curve]["r"]
        self.com = TIPPCommitment(ctx, curve)
        self.pool = ThreadPoolExecutor(max_workers=10)     # independent GPU calls of a phase go out together (one lane each)

    # ---- helpers ----------------------------------------------------------------------------------------
    def _halves(self, buf, size):
        h = len(buf) // 2
        return buf[:h], buf[h:]

    # ---- prove ------------------------------------------------------------------------------------------
    def prove(self, srs, A, B, twist, com, z_ab):
        """A: n G1, B: n G2 (packed affine bytes); com: IppCom (T, U[, ip]) of (A, B) under srs.ck; z_ab: the twisted
        inner product (GT tuple).  Returns the proof dict."""
        ctx, fc, F, r = self.ctx, self.fc, self.F, self.r
        n = srs.n
        g1b, g2b, frb = ctx.g1_bytes, ctx.g2_bytes, ctx.fr_bytes
        from .capi import DeviceBuffer
        t_start = time.perf_counter()
        r_inv = pow(twist, -1, r)
        host = host_scalars()
        # The six vectors of the recursion live in HBM from here to the last round (one allocation, carved up front: a
        # vector of m elements is followed by its folds of m/2, m/4, ... elements): a round's calls take windows of it and
        # write the folded halves next to them, nothing is downloaded until the single final elements.  Behind them the
        # scalar vectors of the device path: twist^i, twist^-i (n Fr each), the quotients q_v (n) and q_w (2 n).
        sizes = [g1b, g2b, g2b, g2b, g1b, g1b]                              # a, b', v1, v2, w1', w2'
        vec_bytes = sum(2 * n * sz for sz in sizes)
        arena = DeviceBuffer(ctx, vec_bytes + (0 if host else 5 * n * frb))
        pending = []                                                        # every call handed to the pool

        def go(fn, *args):
            pending.append(self.pool.submit(fn, *args))
            return pending[-1]
        try:
            base, off = [], 0
            for sz in sizes:
                base.append(off)
                off += 2 * n * sz
            win = lambda k, start, count: arena.view(base[k] + start * sizes[k], count * sizes[k])
            scal = lambda start, count: arena.view(vec_bytes + start * n * frb, count * n * frb)
            twb, twib = twist_vectors(ctx, fc, twist, r_inv, n, None if host else (scal(0, 1), scal(1, 1)))
            # B' = B^(r^i), w' = w^(r^-i): three independent element-wise sweeps, issued together; A, v1, v2 are copied in
            first = [go(ctx.scalar_pairing, 2, B, twb, n, win(1, 0, n)),
                     go(ctx.scalar_pairing, 1, srs.ck.w1, twib, n, win(4, 0, n)),
                     go(ctx.scalar_pairing, 1, srs.ck.w2, twib, n, win(5, 0, n))]
            for k, src in ((0, np.asarray(A)), (2, srs.ck.v1), (3, srs.ck.v2)):
                win(k, 0, n).upload(np.ascontiguousarray(src, dtype=np.uint8))
            for f in first:
                f.result()
            tr = Transcript(r)
            tr.absorb(b"instance", F.encode(com.t), F.encode(com.u), F.encode(z_ab), twist.to_bytes(32, "little"), n.to_bytes(8, "little"))
            rounds, challenges = [], []
            self.round_times = []                                           # (m, pairings s, host s, folds s) per round
            t_rounds = time.perf_counter()
            paired = not os.environ.get("HK_TIPP_SINGLE_ROUNDS")
            pos = gipa_rounds(ctx, F, fc, r, win, n, tr, go, rounds, challenges, self.round_times, paired)
            t_open = time.perf_counter()
            a, b, v1, v2, w1, w2 = (win(k, pos, 1).to_host() for k in range(6))
            tr.absorb(b"final", a, b, v1, v2, w1, w2)
            z = tr.challenge(b"kzg-point")
            # KZG openings of the folded keys (kzg.rs:46-70): quotient polynomials, MSMs over the resident SRS powers, which
            # read the quotients where they lie
            qv, qw = opening_quotients(ctx, fc, challenges, r_inv, z, n, None if host else (scal(2, 1), scal(3, 2)))
            res = srs.resident
            opens = [go(res[k].msm, q, m) for k, q, m in (("h_alpha", qv, n), ("h_beta", qv, n), ("g_alpha", qw, 2 * n),
                                                          ("g_beta", qw, 2 * n))]
            ov1, ov2, ow1, ow2 = (f.result() for f in opens)               # four independent MSMs, issued together
        finally:
            wait(pending)                                                   # no call may outlive the memory it works on
            arena.free()
        self.phase_times = (t_rounds - t_start, t_open - t_rounds, time.perf_counter() - t_open)   # setup, rounds, openings
        proof = dict(rounds=rounds, final_a=a, final_b=b, final_v=(v1, v2), final_w=(w1, w2),
                     open_v=(ov1, ov2), open_w=(ow1, ow2))
        return proof

    # ---- verify -----------------------------------------------------------------------------------------
    def verify(self, vk, com, z_ab, twist, proof, in_gt=False):
        """vk: dict(n, g, h, g_alpha, g_beta, h_alpha, h_beta) - single elements (`tipp_pk.vk()`).  True iff the proof is
        accepted.  in_gt: the caller has established that every round message of the proof lies in GT (hk_gt_check; the
        wire reader `agg_verify.AggProof.deserialize` with a context does) - the fold check then splits its exponents
        along the Frobenius instead of taking the plain chain."""
        ctx, fc, F, r = self.ctx, self.fc, self.F, self.r
        n = vk["n"]
        tr = Transcript(r)
        tr.absorb(b"instance", F.encode(com.t), F.encode(com.u), F.encode(z_ab), twist.to_bytes(32, "little"), n.to_bytes(8, "little"))
        T, U, Z = com.t, com.u, z_ab
        challenges = []
        if len(proof["rounds"]) != n.bit_length() - 1:
            return False
        # the challenges depend on the proof's messages only, so the whole fold check T' = T * prod_k TL_k^(c_k) TR_k^(1/c_k)
        # (likewise U, Z) goes to the GPU as ONE grouped multi-exponentiation (hk_gt_pow_prod: one wavefront per power, then
        # one per product)
        groups = {"T": ([], []), "U": ([], []), "Z": ([], [])}
        for rd in proof["rounds"]:
            tr.absorb(b"round", *(F.encode(rd[k]) for k in ("TL", "UL", "ZL", "TR", "UR", "ZR")))
            c = tr.challenge(b"c")
            c_inv = pow(c, -1, r)
            challenges.append(c)
            for name in "TUZ":
                groups[name][0].extend((rd[name + "L"], rd[name + "R"]))
                groups[name][1].extend((c, c_inv))
        if challenges:
            # the proof's GT members are the prover's word: the plain chain (in_gt = 0), not the Frobenius split that is
            # only a power for elements of order r - unless the caller has checked them (in_gt)
            bases = groups["T"][0] + groups["U"][0] + groups["Z"][0]
            exps = groups["T"][1] + groups["U"][1] + groups["Z"][1]
            f_fold = self.pool.submit(ctx.gt_pow_prod, np.frombuffer(b"".join(F.encode(x) for x in bases), np.uint8),
                                      fc.enc(exps), 2 * len(challenges), bool(in_gt))    # beside the checks below
        else:
            f_fold = None
        a, b = proof["final_a"], proof["final_b"]
        (v1, v2), (w1, w2) = proof["final_v"], proof["final_w"]
        tr.absorb(b"final", a, b, v1, v2, w1, w2)
        z = tr.challenge(b"kzg-point")
        D = F.decode
        go = self.pool.submit
        # every remaining check is independent of the others: the element-wise combinations go out together, then the
        # pairings - the five of the folded instance as one 3 x 3 batch, each KZG check as one 2 x 2 batch
        ch_rev = challenges[::-1]
        chi_rev = [pow(c, -1, r) for c in ch_rev]
        r_inv = pow(twist, -1, r)
        fvz = ipa_polynomial_eval(chi_rev, 1, z, r)
        fwz = pow(z, n, r) * ipa_polynomial_eval(ch_rev, r_inv, z, r) % r
        neg = lambda x: (r - x) % r
        f_inst = go(ctx.pairing_pairs, [a, w1, w2], [b, v1, v2], [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)], 1)
        # Each single-element combination is lo + c * hi: the endomorphism-split fold (K lanes per element, hk_points_fold)
        # instead of a joint 254-step chain (hk_points_lincomb: 4.5 ms in G1, 13 ms in G2 for ONE element).
        # v:  e(g, v' - f_v(z) h) = e(g^tau - z g, pi)
        v_checks = []
        for key, vfin, pi in (("g_alpha", v1, proof["open_v"][0]), ("g_beta", v2, proof["open_v"][1])):
            v_checks.append((go(ctx.points_fold_g2, vfin, vk["h"], neg(fvz), 1),
                             go(ctx.points_fold_g1, vk[key], vk["g"], neg(z), 1), pi))
        # w:  e(w' - f_w(z) g, h) = e(pi, h^tau - z h)
        w_checks = []
        for key, wfin, pi in (("h_alpha", w1, proof["open_w"][0]), ("h_beta", w2, proof["open_w"][1])):
            w_checks.append((go(ctx.points_fold_g1, wfin, vk["g"], neg(fwz), 1),
                             go(ctx.points_fold_g2, vk[key], vk["h"], neg(z), 1), pi))
        f_v = [go(ctx.pairing_pairs, [vk["g"], l1.result()], [l2.result(), pi], [(0, 0), (1, 1)], 1) for l2, l1, pi in v_checks]
        f_w = [go(ctx.pairing_pairs, [l1.result(), pi], [vk["h"], r2.result()], [(0, 0), (1, 1)], 1) for l1, r2, pi in w_checks]
        pi_ = f_inst.result()
        if f_fold is not None:
            pw = f_fold.result()
            T, U, Z = F.mul(D(pw[0]), T), F.mul(D(pw[1]), U), F.mul(D(pw[2]), Z)
        ok = D(pi_[0]) == Z                                                     # the folded instance: e(a, b) = Z
        ok &= F.mul(D(pi_[1]), D(pi_[2])) == T and F.mul(D(pi_[3]), D(pi_[4])) == U
        for f in f_v + f_w:                                                     # both sides of each KZG check
            pr = f.result()
            ok &= D(pr[0]) == D(pr[1])
        return bool(ok)


def verifier_key(ctx, curve, srs):
    """The handful of SRS elements the verifier needs (`tipp_pk.vk()`)."""
    g1b, g2b = ctx.g1_bytes, ctx.g2_bytes
    return dict(n=srs.n, g=srs.g_alpha[:g1b].copy(), h=srs.h_alpha[:g2b].copy(), g_alpha=srs.g_alpha[g1b:2 * g1b].copy(),
                g_beta=srs.g_beta[g1b:2 * g1b].copy(), h_alpha=srs.h_alpha[g2b:2 * g2b].copy(),
                h_beta=srs.h_beta[g2b:2 * g2b].copy())
