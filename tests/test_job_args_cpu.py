"""CPU: the argument rules the job entries share (hekaton_system_amd/csrc/job_args.h) over the refusal cases the GPU tests
name for them (test_exec_tree_gpu, test_stage1_witness_gpu, test_ram_witness_gpu, test_trace_sort_gpu, test_vkd_gpu,
test_r1cs_job_gpu, test_sha_tree_gpu), each beside its nearest valid case.  tests/host_shim/job_args_driver.cpp runs the
table as a stand-alone host program: once as built plainly, once under AddressSanitizer + UBSan in a process of its own."""
import os
import re
import subprocess

import pytest

from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG = "HK_OK", "HK_ERR_ARG"

# the statuses the GPU tests assert of the entries, per rule
EXPECTED = {
    "poseidon_valid": OK, "poseidon_leaf_t5": ARG, "poseidon_leaf_alpha17": ARG, "poseidon_node_t4": ARG,
    "poseidon_node_alpha5": ARG, "poseidon_odd_rounds": ARG, "poseidon_node_odd_rounds": ARG,
    "poseidon_consts_four_short": ARG, "poseidon_consts_one_short": ARG, "poseidon_zero_rounds": ARG,
    "offsets_valid": OK, "offsets_first_one": ARG, "offsets_decreasing": ARG, "offsets_decreasing_last": ARG,
    "rows_valid": OK, "rows_empty_batch": OK, "rows_sub_index_n_sub": ARG, "rows_offsets_first_one": ARG,
    "rows_k_minus_1_entries": ARG, "rows_k_plus_1_entries": ARG, "rows_k_entries": OK,
    "tree_2_1": OK, "tree_8_3": OK, "tree_2p24": OK, "tree_2p25": ARG, "tree_n_sub_0": ARG, "tree_n_sub_1": ARG,
    "tree_n_sub_3": ARG, "tree_n_sub_6": ARG, "tree_depth_minus_1": ARG, "tree_depth_plus_1": ARG,
    "cols_abutting_to_the_end": OK, "cols_any_order": OK, "cols_column_0": ARG, "cols_past_n_v_by_one": ARG,
    "cols_first_past_n_v": ARG, "cols_overlap_0_1": ARG, "cols_overlap_1_2": ARG, "cols_overlap_0_2": ARG,
    "cols_overlap_reordered": ARG,
    "bufs_one_byte": ARG, "bufs_one_byte_swapped": ARG, "bufs_abutting": OK, "bufs_abutting_swapped": OK, "bufs_same": ARG,
    "bufs_inside": ARG, "bufs_null_a": OK, "bufs_null_b": OK,
}


def _build(tmp, name, *flags):
    out = str(tmp / name)
    host_build.build("job_args_driver.cpp", out, "-O1", "-g", "-Wall", "-Werror", *flags)
    return out


def _run(exe, **env):
    p = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **env), timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.fixture(scope="module")
def plain_output(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("job_args"), "job_args_driver"))


def test_refusal_table(plain_output):
    got = dict(line.split() for line in plain_output.splitlines())
    assert len(got) == len(plain_output.splitlines()), "a case is named twice"
    assert got == EXPECTED


def test_refusal_table_under_asan_ubsan(plain_output, tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("job_args_san"), "job_args_driver_san", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    out = _run(exe, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    assert out == plain_output


# ---- the rules exist once, and a carve lambda only carves ------------------------------------------------------------------
CSRC = os.path.join(ROOT, "hekaton_system_amd", "csrc")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cuh", ".h", ".hip"))}


@pytest.mark.parametrize("text,where", [("full_rounds & 1", ["job_args.h", "witness_host.cuh"]),     # hk_poseidon_path keeps its own
                                        ("offsets[i + 1] < offsets[i]", ["job_args.h"]),
                                        ("lo[a] < lo[b] + len[b]", ["job_args.h"])])
def test_a_shared_rule_is_written_once(text, where):
    assert sorted(f for f, src in _sources().items() for _ in range(src.count(text))) == where


def test_carve_lambdas_only_carve():
    """Lane::carve runs its lambda twice and both passes must agree (hk_internal.h): no residency query, no HIP call inside."""
    seen = 0
    for f, src in _sources().items():
        at = src.find("carve([&]")
        while at >= 0:
            depth, k = 0, src.index("{", at)
            for k in range(k, len(src)):
                depth += {"{": 1, "}": -1}.get(src[k], 0)
                if depth == 0:
                    break
            body = src[at:k]
            assert "is_device_ptr" not in body and "hip" not in body and "getenv" not in body, (f, body)
            seen += 1
            at = src.find("carve([&]", k)
    assert seen >= 20


def test_one_staging_idiom():
    """Every entry stages its host-or-device operands through Staged (hk_internal.h): the older helper is gone."""
    assert [f for f, src in _sources().items() if "to_device(" in src] == []


def test_witness_host_asks_residency_outside_loops():
    """One hipPointerGetAttributes per operand, not one per element: no is_device_ptr( in a for / while header or body."""
    src = _sources()["witness_host.cuh"]
    loops = list(re.finditer(r"\b(for|while)\s*\(", src))
    assert loops
    for m in loops:
        depth, k = 0, m.end() - 1
        for k in range(k, len(src)):                      # the header's closing parenthesis
            depth += {"(": 1, ")": -1}.get(src[k], 0)
            if depth == 0:
                break
        end = k + 1
        while src[end].isspace():
            end += 1
        if src[end] == "{":                                # a braced body, else one statement
            for end in range(end, len(src)):
                depth += {"{": 1, "}": -1}.get(src[end], 0)
                if depth == 0:
                    break
        else:
            end = src.index(";", end)
        assert "is_device_ptr(" not in src[m.start():end + 1], src[m.start():end + 1]
