"""The block maps of csrc/evae_tile_map.h (block id -> tile / unit / slice, and the grid size each assumes), checked exhaustively on the
CPU: tests/host/tile_map_check.cpp includes that header alone, is built with the host compiler (with -fsanitize=undefined) and must
exit with status 0.  It covers the contiguous-run map for 1 .. 800 tiles, the unit map for 1 .. 200 units x 1 .. 6 blocks per unit and
the strided-slice map for 1 .. 40 slices x 1 .. 12 tiles: bijection, one XCD (block id & 7) per run / unit / slice, the idle blocks,
and that every grid function returns the smallest grid."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_tile_maps_are_bijections_and_grids_are_smallest(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tile_map_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host", "tile_map_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
