"""Fixtures shared by tests/test_r1cs_check_cpu.py and tests/test_r1cs_check_gpu.py: hand-built rows that exercise the comparison
of hk_r1cs_check itself, and ways to make chosen rows of a synthetic system fail."""


def directed_system(r):
    """(A, B, C rows, z, the rows that fail, {row: (a, b, c)}): the directed rows of tests/test_r1cs_check_gpu.py.
    z: column 0 = 1, then 0, r - 1, and values whose sums and products wrap."""
    z = [1, 0, r - 1, 5, r - 3, 7, 2, (r + 1) // 2]
    A, B, C = [], [], []

    def row(a, b, c):
        A.append(a); B.append(b); C.append(c)
        return len(A) - 1
    ev = lambda lc: sum(c * z[j] for c, j in lc) % r
    bad = []
    row([(1, 3), (r - 1, 3)], [(7, 5), (1 << 31, 4)], [])          # 0: a = z3 + (r - 1) z3: zero reached as a sum that wraps
    a, b = [(1, 3)], [(1, 5)]                                      # 1: c = z_j + z_k >= r as integers, equal to a b = 35
    z.append((35 - z[2]) % r)                                      #    column 8 = 36, so z2 + z8 = r + 35
    assert z[2] + z[8] >= r and (z[2] + z[8]) % r == 35
    row(a, b, [(1, 2), (1, 8)])
    for _ in range(3):                                             # 2 - 4: empty rows, 0 * 0 = 0
        row([], [], [])
    bad.append(row([], [], [(1, 0)]))                              # 5: 0 * 0 != z0, sides (0, 0, 1)
    row([(2, 3)], [(1, 6)], [(4, 3)])                              # 6: 10 * 2 = 20
    bad.append(row([(2, 3)], [(1, 6)], [(4, 3), (1, 0)]))          # 7: the same row with c + 1
    row([(0, 5), (1, 0)], [(r - 1, 2)], [(1, 0)])                  # 8: coefficient 0; (r - 1)(r - 1) = 1
    row([(1 << 31, 7)], [(2, 0)], [(1 << 31, 0)])                  # 9: 2^31 * (r + 1) / 2 * 2 = 2^31
    long_a = [((k * k + 1) % 5 + (r - 2 if k % 7 == 0 else 0), 1 + k % 8) for k in range(40)]
    z.append(ev(long_a) * 3 % r)                                   # column 9
    row(long_a, [(3, 0)], [(1, 9)])                                # 10: one row of 40 terms among rows of <= 2
    row([(1, 1)], [(1, 2)], [(r - 1, 1)])                          # 11: z = 0 on every side
    row([(r - 1, 2)], [(1, 0)], [(1, 0)])                          # 12: (r - 1)(r - 1) = 1 again, as a 1 x 1 row
    sides = {i: (ev(A[i]), ev(B[i]), ev(C[i])) for i in range(len(A))}
    return A, B, C, z, bad, sides


def with_failing_rows(C_rows, rows):
    """C with the term (1, column 0) added to the given rows: z0 = 1, so c shifts by one there and no other row moves."""
    rows = set(rows)
    return [row + [(1, 0)] if i in rows else row for i, row in enumerate(C_rows)]


def resolve_from(A, B, C, z, r, first=0):
    """z with the witness of every row i >= first (the one column of C row i, as tests/util.synthetic_r1cs builds it) set to
    <A_i,z> <B_i,z>, in row order: a satisfying assignment again from that row on."""
    z = list(z)
    ev = lambda lc: sum(c * z[j] for c, j in lc) % r
    for i in range(first, len(A)):
        (one, col), = C[i]
        assert one == 1
        z[col] = ev(A[i]) * ev(B[i]) % r
    return z
