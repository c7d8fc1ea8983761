"""CPU: the column layout, the matrices and the host witnesses of the four portal jobs are, bit for bit, the ones recorded in
tests/golden/portal_layout.json (tests/golden/gen_portal_layout.py wrote it and says what it holds).  The device kernels
write the portal and membership columns by position, so a column that moves in `portal_circuit.py` or in one of the four job
modules has to show here."""
import json

import pytest

from tests.golden import gen_portal_layout as gen

with open(gen.OUT) as f:
    GOLDEN = json.load(f)


def _first_difference(want, got, path):
    """The path of the first entry in which the two records differ, or None."""
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(want) | set(got)):
            if k not in want or k not in got:
                return path + [k], want.get(k, "<absent>"), got.get(k, "<absent>")
            d = _first_difference(want[k], got[k], path + [k])
            if d:
                return d
        return None
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        for i, (w, g) in enumerate(zip(want, got)):
            d = _first_difference(w, g, path + [i])
            if d:
                return d
        return None
    return None if want == got and type(want) is type(got) else (path, want, got)


def test_golden_covers_both_curves():
    assert sorted(GOLDEN) == sorted(gen.CURVES)


@pytest.mark.parametrize("curve", gen.CURVES)
def test_portal_layout(curve):
    got = json.loads(json.dumps(gen.curve_record(curve)))          # through json: the types the file holds
    d = _first_difference(GOLDEN[curve], got, [curve])
    assert d is None, "%s: recorded %r, computed %r" % (" / ".join(str(x) for x in d[0]), d[1], d[2])
