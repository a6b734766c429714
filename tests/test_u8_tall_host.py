"""The block-height rule of the byte layer's forward (u8_fwd_block_rows, csrc/evae_tile_map.h), checked on the CPU:
tests/host/u8_tall_check.cpp includes that header alone, is built with the host compiler (with -fsanitize=undefined) and must exit
with status 0.  Over M = 1 .. 30 000 (every residue mod 64), 1 .. 20 column tiles and 64 / 228 / 256 / 304 CUs the rule returns 128, 256
or 448, returns 448 only where that takes fewer rounds of blocks than 256, is the launcher's earlier choice everywhere else, and
gives 448 at (19 968 rows, 5 tiles, 256 CUs) and 256 at (25 000, 5, 256)."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_block_height_rule_of_the_byte_layer_forward(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "u8_tall_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host", "u8_tall_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
