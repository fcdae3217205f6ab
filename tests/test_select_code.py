"""The in-block select code (csrc/select_code.hpp) on the CPU: the same header the HIP kernels compile, against a bit-by-bit loop."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "select_code_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "select224 ok" in out.stdout and "rrr_select63 ok: 64 classes" in out.stdout
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_block_select_against_bit_loop(tmp_path):
    _build_and_run(tmp_path, "select_code_check", [])


def test_block_select_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "select_code_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
