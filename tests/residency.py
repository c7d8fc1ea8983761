"""What the residency tests share (test_job_residency_gpu, test_entry_residency_gpu): the three placements of a call's inputs,
prefilled device outputs, and the check that every placement gives the same bytes."""
import numpy as np

from hekaton_system_amd import capi

PATTERN = 0xA5
# input k of a call is resident on the device?
PLACEMENTS = {"host": lambda k: False, "device": lambda k: True, "alternating": lambda k: k % 2 == 0}


class _Placed:
    """Puts the inputs of one call where a placement says, in the order they are asked for, and frees the copies."""

    def __init__(self, ctx, placement):
        self.ctx, self.on_device, self.k, self.bufs = ctx, PLACEMENTS[placement], 0, []

    def __call__(self, arr):
        arr = np.ascontiguousarray(arr)
        dev, self.k = self.on_device(self.k), self.k + 1
        if not dev:
            return arr
        self.bufs.append(capi.DeviceBuffer.from_host(self.ctx, arr.reshape(-1).view(np.uint8)))
        return self.bufs[-1]

    def free(self):
        for b in self.bufs:
            b.free()


def _same_everywhere(ctx, run):
    """run(put) -> output bytes, once per placement: all equal, and something was written."""
    got = {}
    for name in PLACEMENTS:
        put = _Placed(ctx, name)
        try:
            got[name] = run(put)
        finally:
            put.free()
    assert not (got["host"] == PATTERN).all()
    for name in PLACEMENTS:
        assert got[name].shape == got["host"].shape and (got[name] == got["host"]).all(), name
    return got["host"]


def _prefilled(ctx, nbytes):
    return capi.DeviceBuffer.from_host(ctx, np.full(max(nbytes, 1), PATTERN, np.uint8))


def _filled(ctx, nbytes, fill):
    """The bytes of a prefilled device buffer after fill(z)."""
    z = _prefilled(ctx, nbytes)
    try:
        fill(z)
        return z.to_host()
    finally:
        z.free()
