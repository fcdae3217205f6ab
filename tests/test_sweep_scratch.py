"""The sorted sweep's scratch layout and control block (csrc/sweep_scratch.hpp) on the CPU: the header the physical pass and the sweep's
driver compile, against the rules a layout keeps and against the expressions it replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sweep_scratch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_layouts_against_their_rules_and_the_expressions_they_replace(tmp_path):
    _build_and_run(tmp_path, "sweep_scratch_check", [])


def test_layouts_with_the_small_variants_chunk(tmp_path):
    """VLG_SWEEP_CHUNK = 512, as the `small` variant compiles it: other turn borders, the same rules"""
    _build_and_run(tmp_path, "sweep_scratch_check_512", ["-DVLG_SWEEP_CHUNK=512"])


def test_layouts_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "sweep_scratch_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
