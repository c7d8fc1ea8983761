"""The verifier of a job's aggregate proof: what `agg_subcircuit_proofs` publishes, checked from public
data alone.  The reference has no such function - aggregation.rs:340 is the prover checking itself with the instance it just
computed - so the equations are restated here from aggregation.rs:138-345 read from the verifier's side:

    AggVerifyingKey     what a verifier keeps per job: the TIPP verifier key (`tipa.verifier_key`), the commitments to the
                        verifying-key columns that `AggProvingKey.new` computes (:97-103), the class of every subcircuit and
                        one GT element e(alpha_c, beta_c) per key class.  No vector of n points.
    AggProof            what the aggregator publishes: com_ab, com_c (:167-168), the 4 x 4 cross terms (:255-263) and the
                        TIPP proof.
    verify_aggregate    twist from the transcript (:219-222); the pairing-product equation (:265-273) with
                        prod_i e(alpha_i, beta_i)^(twist^i) formed as prod_c e(alpha_c, beta_c)^(sigma_c), sigma_c = the sum
                        of twist^i over the subcircuits of class c (hk_class_power_sums: the one computation here that grows
                        with n); s, t (:276-278); com_lr (:171-174, :320-324) and z_lr from the cross terms; `TIPA::verify`.

Both objects have a wire form in ark_serialize.py's framing (u64 little-endian lengths, GT as 12 canonical Fq, points
uncompressed, Fr canonical); the layout is this build's own (PARITY UNPINNED: `ripp` is absent).  Order-r membership of
the GT elements of key and proof is tested where they are READ: `deserialize` with a context runs hk_gt_check over every
member, as it runs hk_points_check over the points.  `verify_aggregate` itself tests nothing of the
kind and by default assumes nothing - every power of a GT element that comes from the proof is taken with the plain chain
(in_gt=False), which is a power for any element of Fq12; `members_in_gt=True` is the caller's statement that the readers'
check (and the caller's own of `super_com`) has been made, and buys the Frobenius-split powers."""
from dataclasses import dataclass

import numpy as np

from .aggregation import IppCom
from .ark_serialize import ArkCodec, Reader, SerializationError, Writer
from .cp_groth16 import CURVE_PARAMS, FrCodec
from .gt import GtField

ACCEPTED = "accepted"
R_INPUT_COUNT = "public input count"
R_INPUT_CHALLENGES = "public input challenges"
R_SIZE = "proof size"
R_PRODUCT = "product equation"
R_TIPP = "tipp"

_ROUND_KEYS = ("TL", "UL", "ZL", "TR", "UR", "ZR")
# the TIPP proof's points in wire order: (key, group, count)
_TIPP_POINTS = (("final_a", 1, 1), ("final_b", 2, 1), ("final_v", 2, 2), ("final_w", 1, 2), ("open_v", 2, 2), ("open_w", 1, 2))
# the TIPP verifier key's points in wire order
_VK_POINTS = (("g", 1), ("h", 2), ("g_alpha", 1), ("g_beta", 1), ("h_alpha", 2), ("h_beta", 2))


def class_power_sums_host(x, class_of, n_classes, r):
    """The mirror of hk_class_power_sums: sums[c] = sum of x^i over the i with class_of[i] == c (ints mod r)."""
    sums, pw = [0] * n_classes, 1
    for c in class_of:
        if not 0 <= c < n_classes:
            raise ValueError("class id out of range")
        sums[c] = (sums[c] + pw) % r
        pw = pw * x % r
    return sums


def cross_terms_bytes(F, z):
    """The 4 x 4 cross terms as `agg_front` appends them to the transcript (Vec<Vec<PairingOutput>>)."""
    return (4).to_bytes(8, "little") + b"".join((4).to_bytes(8, "little") + b"".join(F.serialize(e) for e in row) for row in z)


def class_runs(class_of):
    """class_of as (class, run length) pairs."""
    runs = []
    for c in class_of:
        c = int(c)
        if runs and runs[-1][0] == c:
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    return [tuple(x) for x in runs]


# ---- wire helpers: every failure is a ValueError -----------------------------------------------------------------------
def _put_gt(w, F, x):
    w.put(F.serialize(x))


def _get_gt(r, F):
    b = bytes(r.take(12 * F.nb))
    x = tuple(int.from_bytes(b[i:i + F.nb], "little") for i in range(0, 12 * F.nb, F.nb))
    if any(c >= F.q for c in x):
        raise ValueError("non-canonical field element in a GT member")
    return x


def _put_com(w, F, com, with_ip=False):
    _put_gt(w, F, com.t)
    _put_gt(w, F, com.u)
    if with_ip:
        _put_gt(w, F, com.ip)


def _get_com(r, F, ctx, with_ip=False):
    t, u = _get_gt(r, F), _get_gt(r, F)
    return IppCom(F, t, u, _get_gt(r, F) if with_ip else None, ctx=ctx)


def _get_points(r, codec, group, count):
    return codec.points_from_wire(group, r.take(count * codec.point_size(group)), count)


def _wire(fn):
    """Runs a parser; the cursor's and the codec's own errors (short input, flags, a coordinate >= q) become ValueError."""
    try:
        return fn()
    except SerializationError as e:
        raise ValueError(str(e)) from None


def _check_points(ctx, g1, g2, what):
    """hk_points_check_g1 / _g2 over the points read: on the curve and in the subgroup, or ValueError."""
    if ctx is None:
        return
    for group, pts in ((1, g1), (2, g2)):
        if pts and not ctx.points_check(group, np.concatenate(pts)).all():
            raise ValueError("%s: a G%d point is not on the curve or not in the subgroup" % (what, group))


def _check_gt(ctx, F, members, what):
    """hk_gt_check over the GT members read, in one call: each non-zero and of order dividing r, or ValueError."""
    if ctx is None or not members:
        return
    if not ctx.gt_check(np.frombuffer(b"".join(F.encode(x) for x in members), np.uint8)).all():
        raise ValueError("%s: a GT member is not in the order-r subgroup" % what)


def _com_members(com):
    return [com.t, com.u] + ([com.ip] if com.ip is not None else [])


@dataclass
class AggVerdict:
    ok: bool
    reason: str

    def __bool__(self):
        return self.ok


class AggVerifyingKey:
    """curve, n (a power of two), n_s; tipp_vk: the dict of `tipa.verifier_key`; com_s (n_s), com_h, com_delta0, com_delta1:
    IppCom; class_of: n uint32; alpha_beta[c]: e(alpha_c, beta_c) as a GT tuple."""

    def __init__(self, curve, n, n_s, tipp_vk, com_s, com_h, com_delta0, com_delta1, class_of, alpha_beta):
        self.curve, self.n, self.n_s, self.tipp_vk = curve, int(n), int(n_s), tipp_vk
        self.com_s, self.com_h, self.com_delta0, self.com_delta1 = list(com_s), com_h, com_delta0, com_delta1
        self.class_of = np.ascontiguousarray(class_of, dtype=np.uint32)
        self.alpha_beta = list(alpha_beta)

    @classmethod
    def from_proving_key(cls, apk, tipp_vk):
        """The classes are the distinct (alpha_i, beta_i) of the proving key's columns in order of first appearance; each
        class's pairing is one device call."""
        ctx = apk.ctx
        g1b, g2b = ctx.g1_bytes, ctx.g2_bytes
        alpha, beta = np.asarray(apk.alpha, np.uint8), np.asarray(apk.beta, np.uint8)
        seen, class_of, alpha_beta = {}, [], []
        for i in range(apk.n):
            a, b = alpha[i * g1b:(i + 1) * g1b], beta[i * g2b:(i + 1) * g2b]
            key = a.tobytes() + b.tobytes()
            if key not in seen:
                seen[key] = len(seen)
                alpha_beta.append(apk.F.decode(ctx.multi_pairing(np.ascontiguousarray(a), np.ascontiguousarray(b), 1)))
            class_of.append(seen[key])
        return cls(apk.curve, apk.n, apk.n_s, tipp_vk, apk.com_s, apk.com_h, apk.com_delta0, apk.com_delta1, class_of, alpha_beta)

    def serialize(self):
        F, codec, w = GtField(self.curve), ArkCodec(self.curve), Writer()
        w.u64(self.n)
        w.u64(self.n_s)
        for key, group in _VK_POINTS:
            w.put(codec.points_to_wire(group, self.tipp_vk[key]))
        w.u64(len(self.com_s))
        for com in self.com_s + [self.com_h, self.com_delta0, self.com_delta1]:
            _put_com(w, F, com)
        runs = class_runs(self.class_of)
        w.u64(len(runs))
        for c, length in runs:
            w.u64(c)
            w.u64(length)
        w.u64(len(self.alpha_beta))
        for x in self.alpha_beta:
            _put_gt(w, F, x)
        return w.getvalue()

    @classmethod
    def deserialize(cls, ctx, curve, data):
        """ValueError for what does not parse and - with a context - for a point off its curve or outside the subgroup, or
        a GT member (the n_s + 3 commitments' two each, every alpha_beta[c]) outside the order-r subgroup: one
        hk_points_check per group, then one hk_gt_check.  ctx=None checks neither."""
        return _wire(lambda: cls._read(ctx, curve, data))

    @classmethod
    def _read(cls, ctx, curve, data):
        F, codec, r = GtField(curve), ArkCodec(curve), Reader(data)
        n, n_s = r.u64(), r.u64()
        if n < 2 or n & (n - 1) or n > 1 << 27 or not 1 <= n_s <= 7:
            raise ValueError("n is not a power of two in [2, 2^27], or n_s is not in [1, 7]")
        vk = dict(n=n)
        for key, group in _VK_POINTS:
            vk[key] = _get_points(r, codec, group, 1)
        _check_points(ctx, [vk[k] for k, g in _VK_POINTS if g == 1], [vk[k] for k, g in _VK_POINTS if g == 2], "verifying key")
        if r.u64() != n_s:
            raise ValueError("the number of com_s does not match n_s")
        coms = [_get_com(r, F, ctx) for _ in range(n_s + 3)]
        n_runs = r.u64()
        if n_runs > n:
            raise ValueError("more class runs than subcircuits")
        runs = [(r.u64(), r.u64()) for _ in range(n_runs)]
        n_classes = r.u64()
        if not 1 <= n_classes <= 1024 or any(c >= n_classes or length == 0 for c, length in runs) or \
                sum(length for _, length in runs) != n:
            raise ValueError("the class runs do not cover n subcircuits with classes below the class count")
        alpha_beta = [_get_gt(r, F) for _ in range(n_classes)]
        if r.remaining():
            raise ValueError("trailing bytes")
        _check_gt(ctx, F, [m for com in coms for m in _com_members(com)] + alpha_beta, "verifying key")
        class_of = np.repeat(np.array([c for c, _ in runs], np.uint32), [length for _, length in runs])
        return cls(curve, n, n_s, vk, coms[:n_s], coms[n_s], coms[n_s + 1], coms[n_s + 2], class_of, alpha_beta)


class AggProof:
    """n; com_ab (T, U, inner product), com_c (T, U): IppCom; cross_terms: 4 x 4 GT tuples; tipp: the dict `Tipp.prove`
    returns."""

    def __init__(self, curve, n, com_ab, com_c, cross_terms, tipp):
        self.curve, self.n, self.com_ab, self.com_c, self.tipp = curve, int(n), com_ab, com_c, tipp
        self.cross_terms = [list(row) for row in cross_terms]

    @classmethod
    def from_instance(cls, tipp_proof, inst, curve=None):
        """From what `agg_subcircuit_proofs` returns."""
        curve = curve or inst["com_ab"].ctx.curve
        return cls(curve, inst["size"], inst["com_ab"], inst["com_c"], inst["cross_terms"], tipp_proof)

    def serialize(self):
        F, codec, w = GtField(self.curve), ArkCodec(self.curve), Writer()
        w.u64(self.n)
        _put_com(w, F, self.com_ab, with_ip=True)
        _put_com(w, F, self.com_c)
        w.put(cross_terms_bytes(F, self.cross_terms))
        w.u64(len(self.tipp["rounds"]))
        for rd in self.tipp["rounds"]:
            for k in _ROUND_KEYS:
                _put_gt(w, F, rd[k])
        for key, group, count in _TIPP_POINTS:
            pts = self.tipp[key]
            w.put(codec.points_to_wire(group, np.concatenate([np.asarray(p, np.uint8) for p in pts]) if count > 1 else pts))
        return w.getvalue()

    @classmethod
    def deserialize(cls, ctx, curve, data):
        """ValueError for a length that does not match, trailing bytes, a non-canonical field element, a number of rounds
        other than log2 n, and - with a context - a point off its curve or outside the subgroup, or a GT member (com_ab's
        three, com_c's two, the 16 cross terms, six per round) outside the order-r subgroup.  ctx=None checks neither."""
        return _wire(lambda: cls._read(ctx, curve, data))

    @classmethod
    def _read(cls, ctx, curve, data):
        F, codec, r = GtField(curve), ArkCodec(curve), Reader(data)
        n = r.u64()
        if n < 2 or n & (n - 1) or n > 1 << 27:
            raise ValueError("n is not a power of two in [2, 2^27]")
        com_ab, com_c = _get_com(r, F, ctx, with_ip=True), _get_com(r, F, ctx)
        if r.u64() != 4:
            raise ValueError("the cross terms are not 4 rows")
        cross = []
        for _ in range(4):
            if r.u64() != 4:
                raise ValueError("a row of cross terms is not 4 elements")
            cross.append([_get_gt(r, F) for _ in range(4)])
        if r.u64() != n.bit_length() - 1:
            raise ValueError("the number of rounds is not log2 n")
        rounds = [{k: _get_gt(r, F) for k in _ROUND_KEYS} for _ in range(n.bit_length() - 1)]
        tipp, by_group = dict(rounds=rounds), {1: [], 2: []}
        for key, group, count in _TIPP_POINTS:
            pts = _get_points(r, codec, group, count)
            by_group[group].append(pts)
            size = pts.size // count
            tipp[key] = pts if count == 1 else tuple(pts[j * size:(j + 1) * size].copy() for j in range(count))
        if r.remaining():
            raise ValueError("trailing bytes")
        _check_points(ctx, by_group[1], by_group[2], "proof")
        _check_gt(ctx, F, _com_members(com_ab) + _com_members(com_c) + [e for row in cross for e in row] +
                  [rd[k] for rd in rounds for k in _ROUND_KEYS], "proof")
        return cls(curve, n, com_ab, com_c, cross, tipp)


def verify_aggregate(ctx, avk, super_com, pub_inputs, proof, pt, mem_type=None, trace=None, members_in_gt=False):
    """True iff `proof` (AggProof) aggregates n accepted subcircuit proofs of the job `avk` (AggVerifyingKey) describes, for
    the stage-0 super commitment `super_com` (IppCom) and the public inputs `pub_inputs` (ints).  pt: a fresh
    merlin.Transcript with the aggregator's label.  mem_type (transcript.ROM / RAM): the leading public inputs must be the
    challenges the super commitment hashes to.  Returns AggVerdict(ok, reason): reason names the first check that failed.
    trace: a dict that receives the values the verifier derived (twist, s, t, sigma, z_alpha_beta, com_lr, z_lr).
    members_in_gt: the caller states that every GT member of `avk` and `proof` lies in the order-r subgroup - which
    `AggVerifyingKey.deserialize` and `AggProof.deserialize` establish when they are given a context (hk_gt_check) - AND
    that `super_com`, the caller's own value that no reader has seen, does too (`ctx.gt_check` on its two members where it
    is not the caller's own pairing output).  com_lr, z_lr and TIPP's fold check then take the Frobenius-split powers
    (in_gt = 1) instead of the plain 254-step chain.  The default keeps the plain chain and assumes nothing."""
    from . import tipa
    curve = avk.curve
    F, fc, r_mod = GtField(curve), FrCodec(curve), CURVE_PARAMS[curve]["r"]
    trace = {} if trace is None else trace
    # 1. the statement
    x = [v % r_mod for v in pub_inputs]
    if len(x) != avk.n_s - 1:
        return AggVerdict(False, R_INPUT_COUNT)
    if mem_type is not None:
        from .transcript import RunningEvaluation
        chal = [c % r_mod for c in RunningEvaluation.new(mem_type, super_com, r_mod).challenges]
        if x[:len(chal)] != chal:
            return AggVerdict(False, R_INPUT_CHALLENGES)
    if proof.n != avk.n or len(proof.tipp["rounds"]) != avk.n.bit_length() - 1:
        return AggVerdict(False, R_SIZE)
    # 2. the twist (aggregation.rs:219-222)
    pt.append_serializable(b"AB-commitment", proof.com_ab.serialize_uncompressed())
    pt.append_serializable(b"C-commitment", proof.com_c.serialize_uncompressed())
    pt.append_serializable(b"D-commitment", super_com.serialize_uncompressed())
    twist = trace["twist"] = pt.challenge_scalar(b"r-random-fiatshamir", r_mod)
    # 3. prod_i e(alpha_i, beta_i)^(twist^i) from one pairing per class: the bases come from the key - the caller's own, or read
    # with a context, which checks them (hk_gt_check) - so they are in GT
    n_classes = len(avk.alpha_beta)
    sigma = ctx.class_power_sums(twist, avk.class_of, n_classes)
    zab = ctx.gt_pow_prod(np.frombuffer(b"".join(F.encode(e) for e in avk.alpha_beta), np.uint8), sigma, n_classes, True)
    trace["sigma"], trace["z_alpha_beta_bytes"] = sigma, zab[0].copy()
    z_alpha_beta = trace["z_alpha_beta"] = F.decode(zab[0])
    # 4. the pairing-product equation (:265-273)
    z = proof.cross_terms
    if z[0][0] != F.mul(F.mul(z_alpha_beta, z[1][1]), F.mul(z[2][2], z[3][3])):
        return AggVerdict(False, R_PRODUCT)
    # 5. s, t (:276-278)
    pt.append_serializable(b"cross-terms", cross_terms_bytes(F, z))
    s = trace["s"] = pt.challenge_scalar(b"s-random-fiatshamir", r_mod)
    t = trace["t"] = pt.challenge_scalar(b"t-random-fiatshamir", r_mod)
    s2, s3, t2, t3 = s * s % r_mod, s * s * s % r_mod, t * t % r_mod, t * t * t % r_mod
    # 6. the commitments (:171-174, :320-324): the prepared input's from the key alone; com_lr mixes in the proof's and the
    # statement's, so its powers take the plain chain unless the caller vouches for them (members_in_gt)
    in_gt = bool(members_in_gt)
    com_in = IppCom.lincomb([(avk.com_s[0], None)] + [(avk.com_s[1 + j], x[j]) for j in range(len(x))])
    com_d = IppCom(F, super_com.t, super_com.u, ctx=ctx)
    com_lr = trace["com_lr"] = IppCom.lincomb([(proof.com_ab, None), (com_in, s), (com_d, s2), (proof.com_c, s3), (avk.com_h, t),
                                               (avk.com_delta0, t2), (avk.com_delta1, t3)], in_gt=in_gt)
    # 7. z_lr = prod_ij cross[i][j]^(s^i t^j)
    exps = [pow(s, i, r_mod) * pow(t, j, r_mod) % r_mod for i in range(4) for j in range(4)]
    out = ctx.gt_pow_prod(np.frombuffer(b"".join(F.encode(z[i][j]) for i in range(4) for j in range(4)), np.uint8), fc.enc(exps),
                          16, in_gt)
    z_lr = trace["z_lr"] = F.decode(out[0])
    # 8. TIPA::verify
    T = tipa.Tipp(ctx, curve)
    try:
        ok = T.verify(avk.tipp_vk, com_lr, z_lr, twist, proof.tipp, in_gt=in_gt)
    finally:
        T.pool.shutdown()
    return AggVerdict(True, ACCEPTED) if ok else AggVerdict(False, R_TIPP)
