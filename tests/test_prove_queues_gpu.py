"""GPU: proofs do not depend on how many hardware queues the process has.  The prove lanes' stream
count and role map follow GPU_MAX_HW_QUEUES, which the runtime reads once per process, so each setting runs in a fresh
child process.  There, 8 threads of concurrent hk_prove over two key classes and a direct hk_prove_batch running beside
them must give, byte for byte, what lone sequential hk_prove calls give."""
import os
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (b"QUEUES-CLASS-KEY-A-0123456789abc", b"QUEUES-CLASS-KEY-B-0123456789abc")
ROWS = 4
THREADS = 8


def child():
    """the child process: prints "ok <proofs checked>" or raises"""
    import numpy as np
    from hekaton_system_amd import capi
    from hekaton_system_amd.cp_groth16 import FrCodec, SeededRng, generate_parameters
    from hekaton_system_amd.workload import make_config

    with capi.Context("bn254", 0) as ctx:
        fc = FrCodec("bn254")
        circ = make_config("bn254", "big-merkle-4x1")
        dpks = [generate_parameters(circ, "bn254", SeededRng(s), ctx)[0].upload(ctx) for s in SEEDS]
        zh, rsk = [], []
        for j in range(ROWS):
            circ.set_witness_seed(700 + j)
            zh.append(np.ascontiguousarray(circ.full_assignment_bytes()))
            rsk.append((fc.enc1(0x33 + 11 * j), fc.enc1(0x77 + 5 * j), fc.enc([0x5005 + 19 * j])))

        def prove(k, j):
            r, s, kap = rsk[j]
            a, b, c = dpks[k].prove(zh[j], r, s, kap, n_v=circ.n_v)
            return a.tobytes() + b.tobytes() + c.tobytes()

        want = {(k, j): prove(k, j) for k in range(2) for j in range(ROWS)}      # lone, one after the other
        assert len(set(want.values())) == 2 * ROWS

        batch_out = []

        def batch():
            z = np.concatenate(zh)
            rs = np.concatenate([x[0] for x in rsk])
            ss = np.concatenate([x[1] for x in rsk])
            ks = np.concatenate([x[2] for x in rsk])
            for _ in range(2):
                a, b, c = dpks[1].prove_batch(z, rs, ss, ks, circ.n_v, ROWS)
                batch_out.append([a[j].tobytes() + b[j].tobytes() + c[j].tobytes() for j in range(ROWS)])

        def one(i):
            k, j = i % 2, (i // 2) % ROWS
            return (k, j), prove(k, j)

        side = threading.Thread(target=batch)
        side.start()
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            got = list(pool.map(one, range(48)))
        side.join()
        for i, (key, out) in enumerate(got):
            assert out == want[key], ("hk_prove", i, key)
        assert len(batch_out) == 2
        for rows in batch_out:
            for j, out in enumerate(rows):
                assert out == want[1, j], ("hk_prove_batch", j)
        for d in dpks:
            d.free()
    print("ok %d" % (len(got) + 2 * ROWS))


@pytest.mark.gpu
@pytest.mark.parametrize("queues,serial", [(4, False), (20, False), (4, True)])
def test_proofs_do_not_depend_on_hardware_queues(queues, serial):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues), PYTHONPATH=ROOT)
    env.pop("HK_SERIAL_STREAMS", None)
    if serial:
        env["HK_SERIAL_STREAMS"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.strip().splitlines()[-1] == "ok %d" % (48 + 2 * ROWS), p.stdout[-2000:]


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    sys.path.insert(0, ROOT)
    child()
