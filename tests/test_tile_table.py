"""The register tiles' table builder (csrc/lbm_tile_table.h) on the CPU: a stand-alone program (tests/tile_table_check.cpp)
that includes only that header, built with the host compiler -- under AddressSanitizer and UBSan where the compiler links
their runtimes into the program, plain otherwise -- against the layout written down here from its definition:
  tile = (y / ty) * ntx + x / 64;  slot[tile] = -1 for a tile without a cell, else its rank among the occupied tiles;
  words[((slot * ty) + y % ty) * 64 + x % 64] = the cell's word, every other word 0.
128 columns (two columns of tiles), 8 rows, tiles of 2, 4 and 8 rows."""
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT

NX, NY, NTX = 128, 8, 2
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _cell_sets():
    every = [(x, y) for y in range(NY) for x in range(NX)]
    return {
        "empty": [],
        "corners": [(0, 0), (NX - 1, 0), (0, NY - 1), (NX - 1, NY - 1)],
        "tile_seam": [(63, 5), (64, 5)],
        "every": every,
        "random_third": random.Random(20260).sample(every, len(every) // 3),
    }


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tile_table") / "tile_table_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "advanced-hpc-lbm_amd", "csrc"),
            os.path.join(ROOT, "tests", "tile_table_check.cpp"), "-o", exe]
    built = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    if built.returncode != 0:          # (the sanitizers' runtimes are not installed: the same program, plain)
        print("tile_table_check: built without sanitizers")
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def _expected(ty, cells):
    nty = NY // ty
    occupied = sorted({(y // ty) * NTX + x // 64 for x, y, _ in cells})
    rank = {tile: i for i, tile in enumerate(occupied)}
    slot = [rank.get(tile, -1) for tile in range(NTX * nty)]
    words = [0] * (len(occupied) * ty * 64)
    for x, y, w in cells:
        words[(rank[(y // ty) * NTX + x // 64] * ty + y % ty) * 64 + x % 64] = w
    return slot, words


@pytest.mark.parametrize("ty", [2, 4, 8])
@pytest.mark.parametrize("name", list(_cell_sets()))
def test_layout_matches_its_definition(program, name, ty):
    # (words as the callers make them: distinct, never 0, the top bit in use)
    cells = [(x, y, (0x80000000 if i % 2 else 0) + i + 1) for i, (x, y) in enumerate(_cell_sets()[name])]
    text = "%d %d %d %d\n" % (ty, NTX, NY // ty, len(cells)) + "".join("%d %d %d\n" % q for q in cells)
    run = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.split("\n")
    slot, words = [int(v) for v in lines[0].split()], [int(v) for v in lines[1].split()]
    want_slot, want_words = _expected(ty, cells)
    assert slot == want_slot
    assert words == want_words
    if name == "empty":
        assert slot == [-1] * (NTX * (NY // ty)) and words == []
