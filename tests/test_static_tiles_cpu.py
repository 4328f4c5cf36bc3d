"""The tile walk of the static tuple order (pclean_amd/csrc/static_tiles.h, called by eval.hip: ensure_static_order) on the
host: tests/static_tiles_host/static_tiles_host.cpp is a program with its own main, built once with g++ under
-fsanitize=address,undefined and run directly.  It checks, on planted segment lengths (1, 63, 64, 65, LT - 1, LT, LT + 1,
3 LT + 7, alone and between short neighbours; many short segments followed by one long one; n = 1) and on random ones:

  * the tiles partition [0, n) in order;
  * no wave tile exceeds 64 positions;
  * a segment of at most 64 positions lies in one tile;
  * a segment of more than 64 positions lies in long tiles only — exactly ceil(len / LT) of them, each at most LT positions
    (and of near-equal length), holding nothing but that segment: a long tile holds one tuple id;
  * the 64-position chunks of the streaming pass list every tile in order.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "static_tiles_host", "static_tiles_host.cpp")


def test_static_tile_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "static_tiles_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "all cases passed", lines[-3:]
    ok = [l for l in lines if l.startswith("ok ")]
    assert len(ok) >= 220, len(ok)
    # the planted case of 3 LT + 7 positions was cut into four long tiles, LT itself into one
    assert any(l.startswith("ok one segment of 3079 ") and "long=4" in l for l in ok), ok[:10]
    assert any(l.startswith("ok one segment of 1024 ") and "long=1" in l and "tiles=1 " in l for l in ok), ok[:10]
    assert any(l.startswith("ok one segment of 1025 ") and "long=2" in l for l in ok), ok[:10]
