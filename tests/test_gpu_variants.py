"""The oracle-comparing tests on every build variant and every runtime path (vlg_matching_amd/variants.py).

The default build crosses its tile, run and chunk borders only a few times on the small test texts, and the kept alternates and the
runtime switches are compiled or taken by no other test.  Each variant and each environment run gets ONE fresh child pytest over the
tests in CHILD_TESTS (one after the other: the parent and one child hold the GPU at a time); the child first checks, through
vlg_build_constants, that it loaded the library it was meant to."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

from vlg_matching_amd import variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what every child runs: the constants check first, then the oracle-comparing small-text tests
CHILD_TESTS = ["tests/test_gpu_variants.py::test_loaded_library_has_the_expected_constants"] + [
    "tests/test_gpu_parity.py::" + t for t in (
        "test_search_batch_vs_oracle",
        "test_locate_sorted_sweep_equals_random_access_kernel",
        "test_locate_trail_sharing_equals_plain_locate_and_oracle",
        "test_locate_by_unsampling_equals_sweep_walks_and_oracle",
        "test_window_filter_equals_unfiltered_join_and_oracle",
        "test_window_filter_with_nothing_to_mark",
        "test_window_filter_extreme_gaps",
        "test_window_filter_is_skipped_when_it_cannot_pay",
        "test_join_many_tiles_single_pattern",
        "test_join_batch_vs_oracle_join",
        "test_join_batch_rejects_bad_input_and_chunks",
        "test_k4_list_sort_stand_alone",
        "test_64bit_position_kernels",
        "test_text_order_sa_sampling",
        "test_dense_suffix_array_index",
        "test_rrr_index_variant_equals_plain_and_oracle",
        "test_integer_alphabet_fm_index",
        "test_integer_alphabet_rrr_index",
        "test_pivot_filter_through_the_ladder",
        "test_search_chunked_equals_unchunked",
    )] + ["tests/test_gpu_int_sampling.py::test_int_sweep_first_round_staged_lists", "tests/test_gpu_boundaries.py"]

EXPECT_ENV = "VLG_EXPECT_CONSTANTS"      # set by the runner for its child: the constants the loaded library must report


def test_loaded_library_has_the_expected_constants():
    """vlg_build_constants of the loaded library equals the table: the defaults for the in-tree build, the variant's values in a
    child of the runner below (which would otherwise be testing the default library under another name).  Needs no device."""
    from vlg_matching_amd import capi
    got = capi.build_constants()
    want = json.loads(os.environ[EXPECT_ENV]) if EXPECT_ENV in os.environ else variants.constants(None)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


def test_every_variant_was_built_with_its_constants():
    """build() made every variant of the table, and each reports the constants it was compiled with (loaded in a fresh process)."""
    for name in variants.VARIANTS:
        lib = variants.library(name)
        assert os.path.exists(lib), "variant %s is not built (run __graft_entry__.build())" % name
        code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()))"
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VLG_HIP_LIBRARY=lib), capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert json.loads(out.stdout.strip().splitlines()[-1]) == variants.constants(name), name


def _run_child(capsys, label, env_extra, expect):
    env = dict(os.environ)
    env.update(env_extra)
    env[EXPECT_ENV] = json.dumps(expect)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-p", "no:cacheprovider"] + CHILD_TESTS
    t0 = time.time()
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    wall = time.time() - t0
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    m = re.search(r"(\d+) passed", out.stdout)
    passed = int(m.group(1)) if m else 0
    with capsys.disabled():                          # on the terminal whatever the capture mode: what each child ran and passed
        print("\n[variant %s] %d passed in %.1f s, rc %d; vlg_build_constants %s" % (label, passed, wall, out.returncode,
                                                                                   json.dumps(expect, sort_keys=True)))
    assert out.returncode == 0, "child run %s failed:\n%s" % (label, tail)
    assert re.search(r"\b(failed|error|errors|skipped)\b", out.stdout.splitlines()[-1]) is None, tail
    assert passed > len(CHILD_TESTS), tail


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(variants.VARIANTS))
def test_variant_build_passes_the_oracle_tests(capsys, name):
    lib = variants.library(name)
    assert os.path.exists(lib), "variant %s is not built (run __graft_entry__.build())" % name
    _run_child(capsys, name, {"VLG_HIP_LIBRARY": lib}, variants.constants(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(variants.ENV_RUNS))
def test_env_run_passes_the_oracle_tests(capsys, name):
    env = dict(variants.ENV_RUNS[name])
    env["VLG_HIP_LIBRARY"] = ""                      # the in-tree default library (capi.library_path treats "" as unset)
    _run_child(capsys, name, env, variants.constants(None))
