"""lbm_run_window_stats past 2^31 floats: the 16384 x 16385 lattice of tests/test_large_stats.py with the whole lattice as the
window, lbm_wave<8> with two columns per lane, 8 steps (one pass), every step a sample, device output.  The sums and the
output hold 8 x 16384 x 16385 = 2^31 + 131072 floats: the records of the last window row start at float index 2^31, the
first a signed 32-bit record index in the window-stats flavour (8 * (r * win.nx + q)) could not hold.

Checked as tests/test_large_stats.py checks lbm_run_stats: the last 16 rows and the first 16 rows bit for bit against
tests/test_stats_run.py's stats_of of lbm_run_window over those bands -- existing code, at the same steps, from the same
lattice (lbm_write_state puts it back); the rest of the output holds no NaN and a positive mean pressure.  The case, the
skip rule for room and the child process (torch imported first) are that file's."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from test_large_lattices import PARAMS, _bits, _case
from test_large_stats import BAND, COLS, K, NEED_BYTES, NEED_HOST_BYTES, NX, NY, _host_room
from test_stats_run import p0_of, stats_of
from test_wave_probes import _opts


def test_the_whole_lattice_window_crosses_what_it_claims():
    """The record index of the window-stats flavour, 8 * (r * win.nx + q) in 64 bits: its largest value over this window
    passes 2^31, every one of the last row's is at or past it, and the same expression in 32 bits would have wrapped."""
    last = 8 * ((NY - 1) * NX + (NX - 1))
    assert 8 * (NY - 1) * NX == 2 ** 31 and last + 8 == 8 * NX * NY > 2 ** 31
    assert (last & 0xffffffff) >= 2 ** 31                              # (a 32-bit signed index would have read a negative one)
    assert (2 * 9 * 4 + 2 * 32 + 8) * NX * NY < NEED_BYTES             # two lattices, the sums, the output, the maps


def _large_window_stats_child():
    """Runs in the child process, torch imported first.  Skips, with the reason, where the device or the host has no room."""
    import torch
    import advanced_hpc_lbm_amd as L
    t0 = time.time()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_BYTES:
        print(f"SKIP: {free / 2 ** 30:.1f} GiB of device memory free, the lattices, the sums and the output need {NEED_BYTES / 2 ** 30:.0f} GiB")
        return
    host = _host_room()
    if host is not None and host < NEED_HOST_BYTES:
        print(f"SKIP: {host / 2 ** 30:.1f} GiB of host memory available, the case needs {NEED_HOST_BYTES / 2 ** 30:.0f} GiB")
        return
    opts = _opts(K, COLS)
    prm = L.Param(NX, NY, 10, 10, *PARAMS)
    with L.Lattice(prm, np.zeros((NY, NX), np.int32)) as lat:            # the chunk plan: it depends on neither lattice nor obstacles
        for k, v in opts:
            lat.set_option(k, v)
        lat.run(K)
        plan = {k: int(lat.info(k)) for k in ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows",
                                              "wave_out_cols", "wave_launches")}
    assert plan["engine_last"] == 1 and plan["time_block_active"] == K and plan["march_kernel"] == 1, plan
    assert plan["wave_cols_active"] == COLS and plan["wave_launches"] == 1, plan
    H, W = plan["wave_rows"], plan["wave_out_cols"]
    p, ob, cells = _case(L, NX, NY, NX * 7 + NY, H, W)
    p0 = p0_of(p.density)
    t1 = time.time()
    out = torch.full((NY, NX, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    assert out.numel() > 2 ** 31
    bands = {}
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        av, got = lat.run_window_stats(K, 1, L.Window(0, 0, NX, NY), out=out)
        info = {k: int(lat.info(k)) for k in ("window_stats_in_wave", "window_stats_in_kernel", "window_stats_pieces", "engine_last",
                                              "wave_launches", "wave_rows", "wave_out_cols", "wave_cols_active", "time_block_active")}
        print(f"window stats: {info}")
        assert got is out and info["window_stats_in_wave"] == 1 and info["window_stats_in_kernel"] == 0 and info["engine_last"] == 1, info
        assert info["wave_launches"] == 1 and info["window_stats_pieces"] == 1, info
        assert info["wave_rows"] == H and info["wave_out_cols"] == W, (info, plan)
        assert info["wave_cols_active"] == COLS and info["time_block_active"] == K, info
        t2 = time.time()
        for name, y0 in (("last", NY - BAND), ("first", 0)):
            lat.write_state(cells)
            avw, win = lat.run_window(K, 1, L.Window(0, y0, NX, BAND))
            assert lat.info("window_in_wave") == 1 and win.shape == (K, BAND, NX, 4)
            assert np.array_equal(_bits(avw), _bits(av)), name
            bands[name] = (y0, win)
    torch.cuda.synchronize()
    for name, (y0, win) in bands.items():
        x = out[y0:y0 + BAND].cpu().numpy()
        want = stats_of(win, p0)
        blocked = ob[y0:y0 + BAND] != 0
        assert blocked.any() and np.all(_bits(win[0][blocked][:, 3]) == _bits(p0)), name
        bad = np.argwhere(_bits(x) != _bits(want))
        assert len(bad) == 0, (name, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
    step = 1024
    for r0 in range(0, NY, step):
        part = out[r0:r0 + step]
        assert not bool(torch.isnan(part).any()) and bool((part[..., 3] > 0).all()), r0
    print(f"large window stats ok: set-up {t1 - t0:.1f} s, window stats {t2 - t1:.1f} s, windows and checks {time.time() - t2:.1f} s")


_LARGE = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import conftest
import test_large_window_stats
test_large_window_stats._large_window_stats_child()
"""


@pytest.mark.gpu
def test_window_stats_past_2_31_floats(gpu):
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _LARGE.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    if "SKIP:" in r.stdout:
        pytest.skip(r.stdout[r.stdout.index("SKIP:") + 6:].strip())
    assert "large window stats ok" in r.stdout
