"""CPU: the identity behind the evaluation-basis proving key (csrc/h_basis.cuh) in Python integers, and the host helpers
of csrc/h_basis_plan.h.

The H term of a proof is sum_{i < m-1} h_i H_i with h the reference's witness map.  With scalars standing for the group
elements H_i (the identity is linear in them), the key-side vectors G^ / m^2, G and C^ = C^T G and the prover-side pointwise
product m^2 a'_j b'_j are restated here the way the device code forms them - unscaled inverse transforms, the bit-reversed
load and the decimation-in-time stages of the group transform with their per-stage twiddle tables - and compared with a direct
restatement of the reference's map, for assignments that do NOT satisfy the system: there h_{m-1} != 0, and it is dropped."""
import os
import random
import subprocess

import pytest

from tests import host_build

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # BN254 Fr
GEN = 5
TWO_ADICITY = 28


def _dft(xs, w):
    m = len(xs)
    return [sum(x * pow(w, i * j, R) for i, x in enumerate(xs)) % R for j in range(m)]


def _reference_h(A, B, C, z, n_inst, m):
    """ark-groth16 LibsnarkReduction::witness_map_from_matrices: the m coefficients of h (the prover drops the last)."""
    w = pow(GEN, (R - 1) // m, R)
    winv, minv = pow(w, -1, R), pow(m, -1, R)
    ev = lambda row: sum(c * z[j] for c, j in row) % R
    n_c = len(A)
    a = [ev(r) for r in A] + z[:n_inst] + [0] * (m - n_c - n_inst)
    b = [ev(r) for r in B] + [0] * (m - n_c)
    c = [ev(r) for r in C] + [0] * (m - n_c)
    ifft = lambda v: [x * minv % R for x in _dft(v, winv)]
    coset_fft = lambda co: _dft([x * pow(GEN, i, R) % R for i, x in enumerate(co)], w)
    a2, b2, c2 = (coset_fft(ifft(v)) for v in (a, b, c))
    zinv = pow(pow(GEN, m, R) - 1, -1, R)
    ab = [(x * y - t) * zinv % R for x, y, t in zip(a2, b2, c2)]
    ginv = pow(GEN, -1, R)
    return [x * pow(ginv, i, R) % R for i, x in enumerate(ifft(ab))], (a, b, c)


def _stage_tables(winv, log_m):
    """k_stage_tables: stage s owns tws[(2^s - 1) + j] = (winv^(m / 2^(s+1)))^j, j < 2^s"""
    m = 1 << log_m
    tws = [0] * (m - 1)
    for s in range(log_m):
        ws = pow(winv, m >> (s + 1), R)
        for j in range(1 << s):
            tws[(1 << s) - 1 + j] = pow(ws, j, R)
    return tws


def _group_idft(H, scal, log_m, winv):
    """k_hb_load + k_hb_stage on scalars: bit-reversed load of scal[i] * H[i], then stage by stage in place."""
    m = 1 << log_m
    brev = lambda i: int(format(i, "0%db" % log_m)[::-1], 2) if log_m else 0
    x = [0] * m
    for i in range(m):
        x[brev(i)] = scal[i] * H[i] % R
    tws = _stage_tables(winv, log_m)
    for s in range(log_m):
        half = 1 << s
        for t in range(m // 2):
            pos = t & (half - 1)
            i0 = ((t >> s) << (s + 1)) | pos
            v = x[i0 + half] * tws[half - 1 + pos] % R
            x[i0], x[i0 + half] = (x[i0] + v) % R, (x[i0] - v) % R
    return x


def _eval_basis_h_term(A, B, C, z, n_inst, log_m, H, rows):
    m = 1 << log_m
    w = pow(GEN, (R - 1) // m, R)
    winv, minv = pow(w, -1, R), pow(m, -1, R)
    zinv = pow(pow(GEN, m, R) - 1, -1, R)
    a, b, c = rows
    # prover (QapHost::run_eval): unscaled inverse transform, "* g^j", forward transform, pointwise product
    half = lambda v: _dft([x * pow(GEN, i, R) % R for i, x in enumerate(_dft(v, winv))], w)
    prod = [x * y % R for x, y in zip(half(a), half(b))]
    # key (HBasis::transform, c_columns): H_{m-1} = O
    Hx = H + [0]
    ginv = pow(GEN, -1, R)
    hat = _group_idft(Hx, [zinv * minv ** 3 * pow(ginv, i, R) % R for i in range(m)], log_m, winv)
    G = _group_idft(Hx, [zinv * minv % R] * m, log_m, winv)
    assert hat == [zinv * minv ** 3 * sum(pow(ginv, i, R) * pow(winv, i * j, R) * Hx[i] for i in range(m)) % R for j in range(m)]
    chat = [0] * len(z)
    for row, rw in enumerate(C):
        for coef, k in rw:
            chat[k] = (chat[k] + coef * G[row]) % R
    return (sum(p * g for p, g in zip(prod, hat)) - sum(zk * ck for zk, ck in zip(z, chat))) % R


# (log_m, n_inst, n_c): n_c + n_inst equal to m, and below it (at m = 2 that leaves no constraint: the map is zero there, and
# the identity says so)
SHAPES = [(1, 1, 1), (1, 1, 0), (2, 2, 2), (2, 2, 1), (3, 2, 6), (3, 2, 3), (4, 3, 13), (4, 2, 11)]


@pytest.mark.parametrize("log_m,n_inst,n_c", SHAPES)
def test_identity_on_scalars_for_unsatisfying_assignments(log_m, n_inst, n_c):
    m = 1 << log_m
    rnd = random.Random(1000 * log_m + n_c)
    n_v = n_inst + 5
    row = lambda: [(rnd.randrange(1, R), rnd.randrange(n_v)) for _ in range(rnd.randrange(0, 4))]
    A, B, C = ([row() for _ in range(n_c)] for _ in range(3))
    z = [1] + [rnd.randrange(R) for _ in range(n_v - 1)]
    H = [rnd.randrange(R) for _ in range(m - 1)]
    if log_m >= 3:
        H[2] = 0                                     # a point at infinity in the query
    h, rows = _reference_h(A, B, C, z, n_inst, m)
    assert h[m - 1] != 0 or n_c == 0                 # the system is not satisfied: the dropped coefficient is there
    want = sum(hi * Hi for hi, Hi in zip(h[:m - 1], H)) % R
    assert _eval_basis_h_term(A, B, C, z, n_inst, log_m, H, rows) == want


# ---- host helpers of h_basis_plan.h -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("h_basis")), "h_basis_driver")
    return host_build.build("h_basis_driver.cpp", exe, "-O1", "-Wall", "-Werror")


def _run(driver, mode, text="", *args):
    return subprocess.run([driver, mode, *args], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def _transpose(driver, n_rows, n_cols, row_ptr, col):
    out = _run(driver, "transpose", "%d %d\n%s\n%s\n" % (n_rows, n_cols, " ".join(map(str, row_ptr)), " ".join(map(str, col))))
    if out[0] != "ok 1":
        assert out[0] == "ok 0"
        return None
    return tuple([int(x) for x in line.split()] for line in out[1:4])


def test_transpose_matches_a_python_transpose(driver):
    rnd = random.Random(7)
    for n_rows, n_cols in [(1, 1), (5, 3), (17, 40), (64, 9)]:
        rows = [[rnd.randrange(n_cols) for _ in range(rnd.randrange(0, 5))] for _ in range(n_rows)]
        rows[0] = [0, 0] if n_cols else []           # a duplicate entry stays two entries
        row_ptr, col = [0], []
        for rw in rows:
            col += rw
            row_ptr.append(len(col))
        col_ptr, row, src = _transpose(driver, n_rows, n_cols, row_ptr, col)
        want = [[] for _ in range(n_cols)]
        for r_, rw in enumerate(rows):
            for e, k in enumerate(rw):
                want[k].append((r_, row_ptr[r_] + e))
        assert col_ptr == [sum(len(w) for w in want[:k]) for k in range(n_cols + 1)]
        assert list(zip(row, src)) == [p for w in want for p in w]
        assert all(col[s] == k for k in range(n_cols) for s in src[col_ptr[k]:col_ptr[k + 1]])


def test_transpose_of_an_empty_matrix_and_of_malformed_ones(driver):
    assert _transpose(driver, 3, 4, [0, 0, 0, 0], []) == ([0] * 5, [], [])
    assert _transpose(driver, 2, 2, [0, 1, 2], [0, 2]) is None          # column out of range
    assert _transpose(driver, 2, 2, [0, 2, 1], [0, 1]) is None          # row pointers decrease
    assert _transpose(driver, 2, 2, [1, 1, 2], [0, 1]) is None          # does not start at 0


def test_heavy_column_rule_and_its_override(driver):
    out = _run(driver, "rule", "- 0\n- 256\n- 257\n4 4\n4 5\n0 257\n-3 300\n1 1\n1 2\nabc 257\n")
    default = int(out[0].split()[1])
    assert default == 256
    got = [tuple(map(int, ln.split())) for ln in out[1:] if ln]
    assert got == [(256, 0), (256, 0), (256, 1), (4, 0), (4, 1), (256, 1), (256, 1), (1, 0), (1, 1), (256, 1)]


def test_key_form_switch(driver):
    assert _run(driver, "form", "", "-")[0] == "eval"
    assert _run(driver, "form", "", "coeff")[0] == "coeff"
    assert _run(driver, "form", "", "eval")[0] == "eval"
