"""The key arithmetic of a text window on the FM-index path and the host reference of the cut (csrc/window_cut.hpp) on the CPU,
against a brute-force filter of the list: exhaustively on small texts, at the 32- and 64-bit edges, on lists around a block of 64."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "window_cut_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_keys_and_cut_against_a_filter_of_the_list(tmp_path):
    _build_and_run(tmp_path, "window_cut_check", [])


def test_keys_and_cut_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "window_cut_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
