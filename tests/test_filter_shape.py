"""The window filter's shape and charge (csrc/filter_shape.hpp) on the CPU: the header the planner and FilterPass compile, against the
functions it replaced and against the bytes the filter carves."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "filter_shape_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_shape_and_charge_against_the_functions_they_replace(tmp_path):
    _build_and_run(tmp_path, "filter_shape_check", [])


def test_shape_and_charge_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "filter_shape_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
