"""The tile ranges of the sweep's tail (pclean_amd/csrc/tail_tiles.h, used by sweep.hip: finalize_tail_kernel) on the host:
tests/tail_tiles_host/tail_tiles_host.cpp is a program with its own main, built once with g++ under
-fsanitize=address,undefined and run directly.  For every n_tiles in 0..200 and every workgroup count in 1..n_tiles + 3:

  * the ranges are contiguous and in workgroup order;
  * they cover each tile exactly once;
  * their sizes differ by at most one;
  * surplus workgroups (more workgroups than tiles) get an empty range, and nobody else does.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tail_tiles_host", "tail_tiles_host.cpp")


def test_tail_tile_ranges_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tail_tiles_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "all cases passed", lines[-3:]
    # n_tiles 0..200, workgroup counts 1..n_tiles + 3: sum of (n_tiles + 3)
    assert f"cases {sum(n + 3 for n in range(201))}" in lines, lines[-3:]
    assert "ok 47 tiles over 3 workgroups: 16 16 15" in lines, lines[-3:]
