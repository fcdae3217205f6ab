"""The quad image's block code and tree collapse (csrc/quad_code.hpp) on the CPU: the same header the HIP kernels compile, against a
digit-by-digit loop and against the codes of Huffman-shaped trees."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / (name + ("_san" if extra else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", name + ".cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")
    return out.stdout


@pytest.mark.parametrize("extra", [[], SAN], ids=["plain", "sanitizers"])
def test_quad_block_code_against_digit_loop(tmp_path, extra):
    """all 80 offsets x 4 digits; random, all-equal and digit-3-only words; the derived count of digit 3 (a plain executable: nothing is
    preloaded)"""
    out = _build_and_run(tmp_path, "quad_code_check", extra)
    assert "all-equal ok" in out and "digit 3 ok" in out and "random ok" in out


@pytest.mark.parametrize("extra", [[], SAN], ids=["plain", "sanitizers"])
def test_quad_tree_collapse(tmp_path, extra):
    out = _build_and_run(tmp_path, "quad_tree_check", extra)
    for name in ("sigma2", "sigma3", "spine", "equal256", "flagship28"):
        assert name + " ok" in out
    assert "spine ok: 13 symbols, longest code 12" in out
    assert "equal256 ok: 256 symbols, longest code 8, 255 inner nodes -> 85 quad nodes" in out
