#!/usr/bin/env python3
"""Writes tests/golden/point_codec.json: per curve two twist points whose y lies in the base field, y = (y0, 0) - the only
inputs that reach the second arm of the sign rule of compressed G2 points (decide on y.c1 unless it is zero, then on y.c0).

x is a cube root in Fq2 of y0^2 - b'.  q = 1 mod 3 on both curves, so with q^2 - 1 = 3^s m, 3 not dividing m: for a cube c,
r = c^(1 / 3 mod m) has r^3 = c u with u in the 3-Sylow subgroup (of 3^s elements), and the subgroup is searched for the v
with v^3 = 1 / u.  The smallest y0 >= 2 with a cube are taken.

    python tests/golden/gen_point_codec.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.pyref.curve import Fq2, G2          # noqa: E402
from oracle.pyref.params import CURVES          # noqa: E402


def f2_pow(F, a, e):
    r = F.one
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def cube_root(F, q, c):
    """Some x with x^3 == c in Fq2, or None."""
    order = q * q - 1
    s, m = 0, order
    while m % 3 == 0:
        s, m = s + 1, m // 3
    if f2_pow(F, c, order // 3) != F.one:
        return None
    r = f2_pow(F, c, pow(3, -1, m))
    u = F.mul(f2_pow(F, r, 3), F.inv(c))        # in the 3-Sylow subgroup
    z = (2, 1)
    while f2_pow(F, z, order // 3) == F.one:     # a non-cube: z^m generates the subgroup
        z = (z[0] + 1, 1)
    g = f2_pow(F, z, m)
    v = F.one
    for _ in range(3 ** s):
        if F.mul(f2_pow(F, v, 3), u) == F.one:
            x = F.mul(r, v)
            assert f2_pow(F, x, 3) == c
            return x
        v = F.mul(v, g)
    raise AssertionError("a cube has a cube root")


def main():
    out = {}
    for name, cp in CURVES.items():
        F, G = Fq2(cp.q), G2(cp)
        assert cp.q % 3 == 1
        found = []
        y0 = 2
        while len(found) < 2:
            x = cube_root(F, cp.q, F.sub((y0 * y0 % cp.q, 0), cp.g2_b))
            if x is not None:
                assert G.on_curve((x, (y0, 0)))
                found.append({"y0": y0, "x": ["%x" % x[0], "%x" % x[1]]})
            y0 += 1
        out[name] = {"g2_y_in_base_field": found}
    with open(os.path.join(HERE, "point_codec.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
