"""GPU: the C++ host codecs (hekaton_system_amd/csrc/host/ark_serialize.hpp), compiled with g++ against libhekaton.so, read
the compressed points and proof records the Python codec wrote (the big-int mirror, no device) and write the bytes it
reads back - both curves, over hk_points_compress_* / hk_points_decompress_*."""
import os
import subprocess

import numpy as np
import pytest

from hekaton_system_amd.ark_serialize import ArkCodec, Reader, Writer
from hekaton_system_amd.cp_groth16 import Proof
from tests import point_codec_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_point_codec")
    libdir = os.path.join(ROOT, "hekaton_system_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host_cpp", "test_point_codec.cpp"),
                           "-L" + libdir, "-lhekaton", "-Wl,-rpath," + libdir])
    return out


@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_cpp_codecs_read_and_write_what_python_does(exe, curve, tmp_path):
    cd = ArkCodec(curve)
    arrays = {}
    for group in (1, 2):
        rows = pc.point_family(curve, group)
        lanes = [i for i, r in enumerate(rows) if r[2] in ("sub", "inf")][:24]
        abi = pc.mirror_decompress(curve, group)[1][lanes].reshape(-1).copy()
        arrays[group] = abi
        abi.tofile(tmp_path / ("g%d_abi" % group))
        (tmp_path / ("g%d_wire" % group)).write_bytes(cd.points_to_wire(group, abi, compress=True))
    g1, g2 = arrays[1].reshape(-1, cd.g1b), arrays[2].reshape(-1, cd.g2b)
    proof = Proof(g1[1].copy(), g2[1].copy(), g1[2].copy(), [g1[3].copy(), g1[0].copy()])       # ds[1] is infinity
    assert not g1[0].any()
    for name, a in (("a", proof.a), ("b", proof.b), ("c", proof.c), ("d0", proof.ds[0]), ("d1", proof.ds[1])):
        a.tofile(tmp_path / ("proof_" + name))
    w = Writer()
    cd.write_proof(w, proof, compress=True)
    (tmp_path / "proof_wire").write_bytes(w.getvalue())
    bad = next(r for r in pc.point_family(curve, 1) if r[2] == "no_root")
    (tmp_path / "bad_wire").write_bytes(pc.wire_of(curve, 1, bad[0], bad[1]))
    out = subprocess.run([exe, curve, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "POINT_CODEC_CPP_OK" in out.stdout, out.stdout + out.stderr
    # and the other way round: what the C++ codecs wrote, through the mirror
    for group in (1, 2):
        wire = (tmp_path / ("cpp_g%d_wire" % group)).read_bytes()
        n = arrays[group].size // (cd.g1b if group == 1 else cd.g2b)
        assert cd.points_from_wire(group, wire, n, compress=True).tobytes() == arrays[group].tobytes()
    back = cd.read_proof(Reader((tmp_path / "cpp_proof_wire").read_bytes()), compress=True)
    assert [x.tobytes() for x in (back.a, back.b, back.c, *back.ds)] == [x.tobytes() for x in (proof.a, proof.b, proof.c, *proof.ds)]
