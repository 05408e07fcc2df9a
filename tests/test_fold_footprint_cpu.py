"""util.fold_footprint_violations on synthetic runs (no GPU): the checker of tests/test_gpu_fold_footprint.py finds what it is for.
Host Framed buffers stand in for a fold's planes; each fault is planted in them by hand and must draw exactly the complaint of its
class, naming the plane.  This is the method's positive control: no GPU test provokes anything."""
import numpy as np
import pytest

from util import (FOLD_FILLS, POISON_WORDS, FoldRun, Framed, fold_footprint_violations, fold_guard_bytes, fold_plane, framed, framed_out)

W, ROWS = 12, 5
REFS = {
    "mean": (np.arange(ROWS * W, dtype=np.float32) + 0.5).reshape(ROWS, W),
    "sum": (np.arange(ROWS * W, dtype=np.float64) * 3.25).reshape(ROWS, W),
    "count": np.arange(ROWS * W, dtype=np.uint32).reshape(ROWS, W) + 7,
    # a u8 plane in which both pre-fill bytes are values of the result
    "pick": np.array([0xA5, 0x5A, 0, 255, 3, 0xA5, 0x5A, 9], dtype=np.uint8),
}
ROW_BYTES = {"mean": 4 * W, "sum": 8 * W, "count": 4 * W, "pick": 1}
SLAB = np.arange(4096, dtype=np.uint8)


class _Src:
    """a stand-in for a device source buffer: what was uploaded and what it holds now"""
    kind = "device"

    def __init__(self, which):
        f = framed("host", 0, which, 1024, SLAB, 1024)
        self.uploaded, self._now = f.uploaded, f.uploaded.copy()

    def snapshot(self):
        return self._now


def _runs(spoil=None, skews=None, guard=None):
    """the two runs of a clean fold; spoil(k, planes, src) edits run k's buffers before they are looked at"""
    out = []
    for k in range(len(POISON_WORDS)):
        planes = {}
        for name, ref in REFS.items():
            skew = (skews or {}).get(name, 0)
            p = fold_plane("host", ROW_BYTES[name], ref.nbytes, FOLD_FILLS[k], skew) if guard is None else \
                framed_out("host", guard, ref.nbytes, fill=FOLD_FILLS[k])
            p.body[:] = ref.view(np.uint8).reshape(-1)
            planes[name] = p
        src = _Src(k)
        if spoil:
            spoil(k, planes, src)
        out.append(FoldRun(planes, ROW_BYTES, FOLD_FILLS[k], src))
    return out


def _classes(bad):
    return [c.split(":")[0] for c in bad]


def test_a_clean_pair_draws_no_complaint():
    assert fold_footprint_violations(_runs(), REFS) == []
    # planes off the allocation's alignment (f64: 8 mod 16) are as clean
    assert fold_footprint_violations(_runs(skews={"mean": 4, "sum": 8, "count": 12, "pick": 1}), REFS) == []


def test_the_frames_are_what_they_say():
    p = fold_plane("host", 1 << 20, 64, 0x5A, 8)
    assert p.lo == fold_guard_bytes(1 << 20) + 8 == (4 << 20) + 8 and p.hi == p.lo + 64
    assert (p.snapshot() == 0x5A).all() and fold_guard_bytes(16) == 64 << 10
    assert isinstance(p, Framed) and p.snapshot().size == 2 * p.lo + 64


@pytest.mark.parametrize("plane", list(REFS))
@pytest.mark.parametrize("run", [0, 1])
def test_one_guard_byte_before_the_payload(plane, run):
    def spoil(k, planes, src):
        if k == run:
            planes[plane]._buf[planes[plane].lo - 1] ^= 0xFF
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["guard"] and f"plane {plane}:" in bad[0] and "front guard" in bad[0] and "-1 bytes" in bad[0], bad


@pytest.mark.parametrize("plane", list(REFS))
def test_one_guard_byte_behind_the_payload(plane):
    def spoil(k, planes, src):
        if k == 1:
            planes[plane]._buf[planes[plane].hi] ^= 0xFF
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["guard"] and f"plane {plane}:" in bad[0] and "back guard" in bad[0] and "+0 bytes" in bad[0], bad


@pytest.mark.parametrize("plane,element", [("mean", 17), ("sum", 0), ("count", ROWS * W - 1), ("pick", 2), ("pick", 0), ("pick", 1)])
def test_one_element_left_at_the_pre_fill(plane, element):
    """pick elements 0 and 1 expect 0xA5 and 0x5A: the run with the OTHER pre-fill shows them"""
    unit = REFS[plane].dtype.itemsize

    def spoil(k, planes, src):
        planes[plane].body[element * unit:(element + 1) * unit] = FOLD_FILLS[k]
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["unwritten"] and f"plane {plane}:" in bad[0] and f"first element {element}" in bad[0], bad


def test_a_u8_plane_needs_both_pre_fills():
    runs = _runs()
    runs[1].fill = runs[0].fill
    for name, r in runs[1].planes.items():
        r.front[:] = runs[0].fill
        r.back[:] = runs[0].fill
    bad = fold_footprint_violations(runs, REFS)
    assert _classes(bad) == ["unwritten"] and "plane pick:" in bad[0], bad


@pytest.mark.parametrize("plane,byte", [("mean", 5), ("sum", 8 * W * ROWS - 1), ("count", 0), ("pick", 4)])
def test_one_payload_byte_off_the_reference(plane, byte):
    def spoil(k, planes, src):
        planes[plane].body[byte] ^= 0x01
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["oracle"] and f"plane {plane}:" in bad[0] and f"first at byte {byte}" in bad[0], bad


@pytest.mark.parametrize("plane,byte", [("mean", 4 * W), ("sum", 3), ("count", 4 * W * ROWS - 1), ("pick", 7)])
def test_the_two_poison_runs_differ_in_one_byte(plane, byte):
    def spoil(k, planes, src):
        if k == 1:
            planes[plane].body[byte] ^= 0x40
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["poison"] and f"plane {plane}:" in bad[0] and f"first at byte {byte}" in bad[0], bad


def test_a_changed_source_byte():
    def spoil(k, planes, src):
        if k == 0:
            src._now[1024 + 100] ^= 0x80
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert _classes(bad) == ["source"] and "fill 0" in bad[0] and "first at byte 1124" in bad[0], bad


def test_small_guards_and_missing_runs_are_refused():
    bad = fold_footprint_violations(_runs(guard=4096), REFS)
    assert bad and set(_classes(bad)) == {"guard"} and len(bad) == 2 * len(REFS), bad
    bad = fold_footprint_violations(_runs()[:1], REFS)
    assert "poison" in _classes(bad), bad
    short = dict(REFS, mean=REFS["mean"][:-1])
    bad = fold_footprint_violations(_runs(), short)
    assert _classes(bad) == ["oracle"] and "plane mean:" in bad[0], bad


def test_several_faults_are_all_named():
    def spoil(k, planes, src):
        planes["sum"].body[16:24] = FOLD_FILLS[k]                  # unwritten
        planes["sum"].body[40] ^= 0x02                             # oracle, both runs
        if k == 1:
            planes["count"].body[9] ^= 0x10                        # poison
            planes["pick"]._buf[planes["pick"].hi + 3] = 0         # guard
    bad = fold_footprint_violations(_runs(spoil), REFS)
    assert sorted(_classes(bad)) == ["guard", "oracle", "poison", "unwritten"], bad
    assert sum("plane sum:" in c for c in bad) == 2 and sum("plane count:" in c for c in bad) == 1 and sum("plane pick:" in c for c in bad) == 1
