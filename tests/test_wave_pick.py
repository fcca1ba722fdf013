"""What one lbm_wave launch on a lattice alone runs, and what a group of K steps is told (csrc/lbm_wave_pick.h), on the CPU: a
stand-alone program (tests/wave_pick_check.cpp) that includes only that header, built with the host compiler -- under
AddressSanitizer and UBSan where the compiler links their runtimes into the program, plain otherwise.

wave_pick is held, for all 256 combinations of its inputs, to the rules launch_wave was written to (its comment, as it stood
when the choice was an if / else chain inside it):
  - with forces wanted (bodies) and a counted cell, the force flavour on the force map; no counted cell, the plain kernel;
  - with probes wanted, the probe flavour on the probe map, or the force-and-probe flavour on the force-and-probe map; a group
    without a sample step runs what it would run without probes;
  - with fields wanted (no forces, no probes beside them: refused), the field flavour -- a window's: the window flavour -- for
    a group that holds a sample step, the plain kernel for one that holds none;
  - under a schedule, the driven flavour; beside forces or probes EVERY group runs the driven force-and-probe flavour, a sample
    step in it or not, on the map that marks what is wanted; beside fields: refused.
wave_group is held to: step s (from 1) is a probe sample iff s >= pfirst and (s - pfirst) % every == 0, row (s - pfirst) // every;
a field sample iff s % every == 0, slot s // every - 1; level l of the group from step tt applies the pair of step tt + l, the
run's last level none."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
FLAVOURS = ["plain", "force", "probe", "force_probe", "field", "window", "driven", "driven_observed"]   # (the enum's order)
MAPS = ["blocked", "fmap", "pmap", "fpmap"]
INPUTS = ["schedule", "bodies", "counted", "probes", "psample", "fields", "fsample", "window"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wave_pick") / "wave_pick_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "advanced-hpc-lbm_amd", "csrc"),
            os.path.join(ROOT, "tests", "wave_pick_check.cpp"), "-o", exe]
    built = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    if built.returncode != 0:          # (the sanitizers' runtimes are not installed: the same program, plain)
        print("wave_pick_check: built without sanitizers")
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def _refused(i):
    """fields beside forces or probes, or fields under a schedule -- and nothing else"""
    return i["fields"] and (i["bodies"] or i["probes"] or i["schedule"])


def _expected(i):
    """(flavour, map, force arguments filled) of an admitted combination; a sample flag or `window` beside no want of its
    kind says nothing"""
    counted = i["bodies"] and i["counted"]
    psample, fsample = i["probes"] and i["psample"], i["fields"] and i["fsample"]
    marked = {(False, False): "blocked", (True, False): "fmap", (False, True): "pmap", (True, True): "fpmap"}
    if i["schedule"] and (i["bodies"] or i["probes"]):
        return "driven_observed", marked[counted, i["probes"]], counted
    if i["schedule"]:
        return "driven", "blocked", False
    if fsample:
        return ("window" if i["window"] else "field"), "blocked", False
    if psample:
        return ("force_probe" if counted else "probe"), marked[counted, True], counted
    if counted:
        return "force", "fmap", True
    return "plain", "blocked", False


def test_every_combination_of_the_inputs(program):
    run = subprocess.run([program, "pick"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    rows = [line.split() for line in run.stdout.splitlines()]
    assert len(rows) == 256
    seen, reached = set(), set()
    for row in rows:
        bits, (flavour, wmap, forces, refused) = [int(v) for v in row[:8]], [int(v) for v in row[9:]]
        seen.add(tuple(bits))
        i = dict(zip(INPUTS, (bool(b) for b in bits)))
        assert bool(refused) == _refused(i), i
        if refused:
            continue
        assert (FLAVOURS[flavour], MAPS[wmap], bool(forces)) == _expected(i), i
        reached.add(FLAVOURS[flavour])
    assert seen == set(itertools.product((0, 1), repeat=8))
    assert reached == set(FLAVOURS)


def _group_cases():
    cases = []
    for K in (4, 6, 8):
        for nsteps in (K, 2 * K + 5):
            for every in (1, 3, K, K + 1):
                for pfirst in (1, every):
                    cases.append((K, nsteps, every, pfirst, every, 7, 1))
    # probes and fields of different periods; one observer alone; no schedule
    cases += [(8, 21, 3, 2, 5, 11, 1), (6, 17, 0, 0, 4, 3, 1), (4, 13, 2, 1, 0, 0, 1), (8, 21, 3, 3, 4, 7, 0)]
    return cases


def test_groups_match_their_definition(program):
    cases = _group_cases()
    text = "".join("%d %d %d %d %d %d %d\n" % c for c in cases)
    run = subprocess.run([program, "groups"], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    blocks = run.stdout.split("end\n")
    assert len(blocks) == len(cases) + 1 and blocks[-1] == ""
    for (K, nsteps, pevery, pfirst, fevery, fstride, driven), block in zip(cases, blocks):
        lines = [line.split() for line in block.splitlines()]
        assert [int(line[0]) for line in lines] == list(range(0, nsteps - K + 1, K))
        for line in lines:
            tt, pmask, prow, fmask, fslot = (int(v) for v in line[:5])
            drv, was_driven = [float(v) for v in line[5:5 + 2 * K]], int(line[5 + 2 * K])
            steps = range(tt + 1, tt + K + 1)
            psamples = [s for s in steps if pevery and s >= pfirst and (s - pfirst) % pevery == 0]
            fsamples = [s for s in steps if fevery and s % fevery == 0]
            assert pmask == sum(1 << (s - tt - 1) for s in psamples)
            assert fmask == sum(1 << (s - tt - 1) for s in fsamples)
            assert prow == ((psamples[0] - pfirst) // pevery if psamples else 0)
            assert fslot == ((fsamples[0] // fevery - 1) * fstride if fsamples else -1)
            want = []
            for s in steps:        # (step s, 0-based, of the schedule is (s + 0.25, -s - 0.5); beyond the run and off a schedule: zeros)
                want += [s + 0.25, -s - 0.5] if driven and s < nsteps else [0.0, 0.0]
            assert drv == want
            assert was_driven == driven
        if nsteps % K == 0 and driven:      # the zeroed last level, looked at on its own
            assert lines[-1][5 + 2 * K - 2:5 + 2 * K] == ["0", "0"]
