"""Deep slabs (-m gpu): the chain kernel templates of util.DEEP_CASES on runs of windows whose absolute sample indices lie around 2^32, around 2^33 and at
the end of a described stream of 2^34 + 12 345 samples (window indices past 2^32 where the stride is 2), byte for byte against the oracle.

The referee (util.deep_reference) is an oracle chain over the slab alone whose shift stages use the reference's f32 multipliers of the
ABSOLUTE indices, planted through override_shift.  tests/test_deep_slabs_cpu.py holds the slabs to their conditions on the reference
alone; the one that matters here: no slab holds an ambiguous NCO multiplier component (util.ambiguous_components is empty over every
shift stage's span).  The NCO rule therefore has nothing to excuse and is not consulted: EVERY output byte equals the oracle's, for
norms, glyph codes, bucket digits, marks and write blocks, behind a shift or not.  A 32-bit truncation of a sample index, a window
index, an NCO row index or a byte offset in any of the kernels below changes whole windows.

Each case (util.DEEP_CASES) is asserted to run on its intended kernel, with the second-order NCO chosen by the plan itself from the
described length, and each of its runs goes through: pageable host memory, a device-resident slab that is larger than the run reads,
a start one window inside a tile (asserted to be off the kernel's row grid wherever it has one and a window can be), the same from a
slab that begins one sample earlier (asserted off every load vector: the per-sample fallback kernel), and, for the cases marked `paths`, 64 KiB host chunks.  Plans are created with explicit options
(never the auto policy: a 2^34-sample description makes it compile), so the QD_* names of the test matrix do not reach them."""
import os

import numpy as np
import pytest

from test_gpu_parity import record_observed
from util import DEEP_CASES, FMT_BYTES, deep_geometry, deep_reference

pytestmark = pytest.mark.gpu


def _plan(engine, case, rng=None, **opt_kw):
    policy = {"generic": engine.KERNEL_GENERIC, "specialise": engine.KERNEL_SPECIALISE, "builtin": engine.KERNEL_NO_PLAN_TIME}[case.policy]
    opts = engine.plan_options(kernel_policy=policy, tile_hint=case.tile_hint, **opt_kw)
    kw = dict(width=case.W, stride=case.S, epilogue=case.epilogue, options=opts, rng=rng)
    if len(case.lowpasses) > 1 or (case.stages and case.stages[-1][0] == "shift" and case.lowpasses):
        kw["stages"] = case.stages
    else:
        kw.update(shift_hz=dict(case.stages).get("shift"), lowpass=dict(case.stages).get("lowpass"))
    return engine.Plan(case.fmt, case.sr, case.N, **kw)


_SPARK, _SPARK0, _PIPE3, _FAST_P1 = 524288, 2097152, 32768, 8


def _row_grid(case, info):
    """(unit, what): the grid a launch's first window must sit on to stay on the plan's fast kernel, as launch_chain (quadrs_hip.hip)
    tests it — in source samples, or in windows for the interleaved launches; None where any start does.  Runtime-geometry kernels
    (kind 0) and k_spark0 take any window; the wave-local kernels start on their 512-sample NCO rows behind a shift and on a load vector
    otherwise; the interleaved launches on R * (512 / W) windows, which is the plan's tile_windows; the three-stage kernels and the
    row-aligned phase 1 (flag 8) on rows of nt * (samples per load), nt the row-loading threads (the three-stage kernels add 512)."""
    flags, spl = int(info.kernel_flags), (2 if case.fmt == 0 else 4)
    if int(info.kernel_kind) == 0 or flags & _SPARK0:
        return None, "any start"
    if flags & _SPARK:
        if case.S < case.W:
            return (int(info.tile_windows), "windows") if case.shifted else (None, "any start")
        return (512 if case.shifted else spl), "samples"
    if flags & _PIPE3:
        return (int(info.threads) - 512) * spl, "samples"
    if flags & _FAST_P1:
        return int(info.threads) * spl, "samples"
    return None, "any start"


def _differing(case, got, ref, n):
    """windows of the run whose bytes differ from the oracle's"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case.name, got.dtype, got.shape, ref.dtype, ref.shape)
    return np.flatnonzero((np.ascontiguousarray(got).view(np.uint8).reshape(n, -1) != ref.view(np.uint8).reshape(n, -1)).any(axis=1))


def _host(p, case, raw, base, w0, n):
    first, count = p.src_range(w0, n)
    bps = FMT_BYTES[case.fmt]
    assert base <= first and (first + count - base) * bps <= raw.size, (case.name, base, first, count, raw.size)
    return p.run_host(raw[(first - base) * bps:(first - base + count) * bps], w0, n, src_first=first)


@pytest.mark.parametrize("case", DEEP_CASES, ids=lambda c: c.name)
def test_deep_runs_equal_the_oracle_byte_for_byte(engine, oracle, case):
    import torch
    total, complete, raw_step, raw_per_window = deep_geometry(engine, case)
    runs = [(depth, w0, n) + deep_reference(oracle, case, depth, w0, n) for depth, w0, n in case.runs(total)]
    rng = None if case.sink not in ("glyph", "mark") else runs[0][6]
    plans = {}

    def plan_for(rng_, **kw):
        key = (rng_, tuple(sorted(kw.items())))
        if key not in plans:
            plans[key] = _plan(engine, case, rng=rng_, **kw)
        return plans[key]
    p = plan_for(rng)
    name, info = p.kernel_name(), p.info
    print(f"{case.name}: {name} | kind {int(info.kernel_kind)} flags {int(info.kernel_flags)} tile_windows {int(info.tile_windows)} "
          f"threads {int(info.threads)} windows {int(p.n_windows)}")
    assert p.n_windows == total and p.complete_windows() == complete
    assert (int(info.raw_step), int(info.raw_per_window)) == (raw_step, raw_per_window)
    if not os.environ.get("QD_NO_FIXED"):
        assert case.family(info, name), (case.name, name, int(info.kernel_kind), int(info.kernel_flags))
        assert max(int(info.tile_windows), 1) == case.tile, (case.name, int(info.tile_windows))
    if case.shifted and "k_cascade" not in name:            # (the cascade kernels have the second-order NCO only: their name carries no order)
        assert "nco 2" in name, name                        # second order, chosen from the described length alone
    checked = differing = 0
    kinds = []
    spl = 2 if case.fmt == 0 else 4
    grid, unit = _row_grid(case, info)
    off_grid = []
    for depth, w0, n, raw, base, ref, used in runs:
        p = plan_for(used)                                  # the mark sink's min follows the run's reference
        assert w0 % case.tile == 0 and p.src_range(w0, n) == (w0 * raw_step, (n - 1) * raw_step + raw_per_window)
        bps = FMT_BYTES[case.fmt]
        per = ref.shape[0] // n
        got = {"host": _host(p, case, raw, base, w0, n)}
        src = torch.from_numpy(raw.copy()).cuda()
        out = torch.full((ref.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        p.run_device(src, out, w0, n, src_first=base, src_count=raw.size // bps)
        torch.cuda.synchronize()
        got["device"] = out.cpu().numpy().view(ref.dtype).reshape(ref.shape)
        got["inside a tile"] = _host(p, case, raw, base, w0 + 1, n - 1)
        # the same windows from a slab that starts one sample earlier, off every load vector: the per-sample kernel (fn_unaligned)
        first, count = p.src_range(w0 + 1, n - 1)
        # where the plan's kernel is row-aligned, the start inside the tile is off its grid (the launch falls to the per-sample kernel)
        # unless every window starts on a row; the odd slab start is off every load vector, whatever the grid
        at = w0 + 1 if unit == "windows" else first
        if grid is not None and (unit == "windows" or raw_step % grid):
            assert at % grid != 0, (case.name, depth, at, grid, unit)
        off_grid.append(grid is not None and at % grid != 0)
        assert (first - 1) % spl != 0, (case.name, depth, first)
        got["inside a tile, odd slab start"] = p.run_host(raw[(first - 1 - base) * bps:(first - base + count) * bps], w0 + 1, n - 1, src_first=first - 1)
        if case.paths:
            small = plan_for(used, chunk_bytes=1 << 16)
            got["64 KiB chunks"] = _host(small, case, raw, base, w0, n)
            assert small.stats().chunks >= 3, (case.name, int(small.stats().chunks))
        for kind, g in got.items():
            r, m = (ref[per:], n - 1) if kind.startswith("inside a tile") else (ref, n)
            bad = _differing(case, g, r, m)
            checked += m
            differing += bad.size
            kinds.append(kind)
            assert bad.size == 0, (case.name, depth, kind, f"windows {w0} + {bad[:8].tolist()} differ from the oracle")
    record_observed(f"deep slab {case.name}", kernel=name[:96], runs=[(d, w0, n) for d, w0, n, *_ in runs], paths=sorted(set(kinds)),
                    windows=checked, differing=differing, row_grid=[grid, unit], inside_tile_start_off_the_grid=off_grid)
    for q in plans.values():
        q.close()
