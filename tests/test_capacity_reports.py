"""CPU: the mailbox for capacity reports that reached the wrong owner (ops.CapacityReports; bindings/ts/capacity_reports.js mirrors it).  The library reports
a truncated tile-entry list device-wide, to whoever waits first (csrc/api.hip: deferred_checks); a Trainer and a Viewer on one device each keep the
reports about their own passes and leave the others for the owner (dropped, such a report was lost to the owner)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS_JS = os.path.join(ROOT, "bindings", "ts", "capacity_reports.js")   # (plain JavaScript: loads without the N-API addon)


def _report(*passes):
    return RuntimeError("[wdgs -3] tile entries overflow: " + "; ".join(f"{n} entries needed, max_tile_entries = 1048576 (forward pass {h:#x})" for n, h in passes)
                        + " (raise wdgs_tiled_forward_config.max_tile_entries)")


def test_reports_wait_for_the_owner_of_the_passes_they_name():
    from webdgs_amd.ops import CapacityReports
    box = CapacityReports(keep=3)
    trainer_passes, viewer_pass = [0x5000, 0x5100, 0x5200], [0x7000]
    assert CapacityReports.passes_named(_report((2_000_000, 0x5100), (1_500_000, 0x7000))) == {0x5100, 0x7000}
    assert box.take(trainer_passes) is None
    # the viewer's read consumed a report about the trainer's pass: left for the trainer, not for the viewer
    box.post(_report((2_000_000, 0x5100)))
    assert box.take(viewer_pass) is None
    e = box.take(trainer_passes)
    assert e is not None and "0x5100" in str(e) and box.take(trainer_passes) is None
    # a report that names passes of both is the first owner's who looks; the oldest matching one comes first; only `keep` are kept
    for n in (1, 2, 3, 4):
        box.post(_report((n, 0x7000)))
    assert len(box.pending) == 3
    assert "1 entries" not in str(box.pending[0]) and "2 entries" in str(box.take(viewer_pass))
    # a step skipped on every rank names no pass: nobody's
    box.post(RuntimeError("an optimizer step was skipped on every rank"))
    assert box.take(trainer_passes) is None


def test_the_node_host_keeps_the_same_mailbox():
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not available")
    src = """
      const { CapacityReports } = require(process.argv[1]);
      const rep = (n, h) => new Error(`tile entries overflow: ${n} entries needed, max_tile_entries = 1048576 (forward pass 0x${h.toString(16)})`);
      const box = new CapacityReports(3), out = [];
      box.post(rep(2000000, 0x5100));
      out.push(box.take([0x7000n]) === null, /0x5100/.test(box.take([0x5000n, 0x5100n]).message), box.take([0x5100n]) === null);
      for (const n of [1, 2, 3, 4]) box.post(rep(n, 0x7000));
      out.push(box.pending.length === 3, /^tile entries overflow: 2 /.test(box.take([0x7000]).message));
      console.log(JSON.stringify(out));
    """
    r = subprocess.run([node, "-e", src, REPORTS_JS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [True] * 5


# ---- the report parser (ops.CapacityReports.parse / split; capacity_reports.js mirrors it), on exact copies of the library's two message forms (csrc/api.hip)
def _line(needed, capacity, handle):
    return f"{needed} entries needed, max_tile_entries = {capacity} (forward pass {handle:#x})"   # "%u entries needed, max_tile_entries = %u (forward pass %p)"


def _deferred(*passes):
    """deferred_checks: "tile entries overflow: %s (raise wdgs_tiled_forward_config.max_tile_entries)" over the passes' lines joined by "; "."""
    return RuntimeError("[wdgs -3] tile entries overflow: " + "; ".join(_line(*p) for p in passes) + " (raise wdgs_tiled_forward_config.max_tile_entries)")


def _checked(needed, capacity, handle):
    """wdgs_tiled_forward_check: "tile entries overflow: %u entries needed, max_tile_entries = %u (forward pass %p)"."""
    return RuntimeError("[wdgs -3] tile entries overflow: " + _line(needed, capacity, handle))


PASSES = [(1_924_441, 1_921_024, 0x7f3a12345000), (0xFFFFF000, 1 << 20, 0x7f3a12346f80), (1_048_577, 1_048_576, 0x55d0c0ffee10), (3, 2, 0x7f3a00000010)]
SKIPPED = "[wdgs -3] an optimizer step was skipped on every rank: tile entries overflowed on another rank (its own error names the size)"


@pytest.mark.parametrize("n", [1, 2, 4])
def test_parse_reads_every_pass_of_a_deferred_report_in_order(n):
    from webdgs_amd.ops import CapacityReports, Overflow
    got = CapacityReports.parse(_deferred(*PASSES[:n]))
    assert got == [Overflow(*p) for p in PASSES[:n]]
    assert [(o.needed, o.capacity, o.handle) for o in got] == PASSES[:n]
    assert CapacityReports.passes_named(_deferred(*PASSES[:n])) == {p[2] for p in PASSES[:n]}


def test_parse_reads_the_single_pass_form_and_nothing_from_other_errors():
    from webdgs_amd.ops import CapacityReports, Overflow
    assert CapacityReports.parse(_checked(*PASSES[1])) == [Overflow(0xFFFFF000, 1 << 20, 0x7f3a12346f80)]
    assert CapacityReports.parse(RuntimeError(SKIPPED)) == []
    assert CapacityReports.parse(RuntimeError("[wdgs -1] wdgs_buffer_create: size must be positive")) == []


def test_split_tells_own_passes_from_other_owners():
    from webdgs_amd.ops import CapacityReports, Overflow
    a, b, c = PASSES[:3]
    assert CapacityReports.split(_deferred(a, b), [a[2], b[2], 0x1234]) == ([Overflow(*a), Overflow(*b)], False)   # own handles only
    assert CapacityReports.split(_deferred(a, b), [c[2]]) == ([], True)                                            # others only
    assert CapacityReports.split(_deferred(a, b, c), iter([b[2]])) == ([Overflow(*b)], True)                       # both (any iterable of handles)
    assert CapacityReports.split(_deferred(a), []) == ([], True)                                                   # an empty own set
    assert CapacityReports.split(RuntimeError(SKIPPED), [a[2]]) == ([], False)                                     # names no pass: nobody's


def test_the_node_host_parses_and_splits_the_same():
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not available")
    src = """
      const { CapacityReports } = require(process.argv[1]);
      const passes = JSON.parse(process.argv[2]).map((p) => ({ needed: p[0], capacity: p[1], handle: BigInt(p[2]) }));
      const line = (p) => `${p.needed} entries needed, max_tile_entries = ${p.capacity} (forward pass 0x${p.handle.toString(16)})`;
      const deferred = (ps) => new Error('[wdgs -3] tile entries overflow: ' + ps.map(line).join('; ') + ' (raise wdgs_tiled_forward_config.max_tile_entries)');
      const same = (got, want) => got.length === want.length && got.every((o, i) => o.needed === want[i].needed && o.capacity === want[i].capacity && o.handle === want[i].handle);
      const [a, b, c] = passes, out = [];
      for (const n of [1, 2, 4]) out.push(same(CapacityReports.parse(deferred(passes.slice(0, n))), passes.slice(0, n)));
      out.push(same(CapacityReports.parse(new Error('[wdgs -3] tile entries overflow: ' + line(b))), [b]));
      out.push(CapacityReports.parse(new Error(process.argv[3])).length === 0, CapacityReports.parse(new Error('[wdgs -1] wdgs_buffer_create: size must be positive')).length === 0);
      let s = CapacityReports.split(deferred([a, b]), [a.handle, b.handle, 0x1234]); out.push(same(s.mine, [a, b]) && s.others === false);
      s = CapacityReports.split(deferred([a, b]), [c.handle]); out.push(s.mine.length === 0 && s.others === true);
      s = CapacityReports.split(deferred([a, b, c]), [b.handle]); out.push(same(s.mine, [b]) && s.others === true);
      s = CapacityReports.split(deferred([a]), []); out.push(s.mine.length === 0 && s.others === true);
      console.log(JSON.stringify(out));
    """
    r = subprocess.run([node, "-e", src, REPORTS_JS, json.dumps([[n, c, hex(h)] for n, c, h in PASSES]), SKIPPED],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [True] * 10


# ---- settle: the one routine every owner of forward passes waits through (ops.CapacityReports.settle; capacity_reports.js mirrors it), with a fake wait
A, B, C = PASSES[:3]          # a and c are the owner's passes, b is another owner's
OWN = [A[2], C[2]]
GROWN = [((1 << 20, (1 << 20) + 1), 2 << 20), ((1 << 20, 4_000_000), 6_000_000), ((0xFFFFF000, 5_000_000_000), 0xFFFFF000), ((3, 3), 6)]


def _raises(error):
    def wait():
        if error is not None:
            raise error
    return wait


def _capacity(*passes):
    from webdgs_amd.ops import CapacityError
    return CapacityError(-3, "tile entries overflow: " + "; ".join(_line(*p) for p in passes) + " (raise wdgs_tiled_forward_config.max_tile_entries)")


def test_settle_returns_nothing_when_nothing_was_reported():
    from webdgs_amd.ops import CapacityReports, Settled
    box = CapacityReports()
    assert box.settle(OWN, _raises(None)) == Settled([], False, None) and box.pending == []


def test_settle_keeps_a_report_about_own_passes_whole():
    from webdgs_amd.ops import CapacityReports, Overflow
    box, report = CapacityReports(), _capacity(C, A)
    got = box.settle(OWN, _raises(report))
    assert got.mine == [Overflow(*C), Overflow(*A)] and got.foreign is False and got.error is report   # (the report's order)
    assert box.pending == []


def test_settle_leaves_a_report_about_others_for_them():
    from webdgs_amd.ops import CapacityReports, Overflow
    box = CapacityReports()
    got = box.settle([A[2]], _raises(_capacity(B, C)))
    assert got.mine == [] and got.foreign is True and got.error is None
    assert len(box.pending) == 1 and CapacityReports.parse(box.pending[0]) == [Overflow(*B), Overflow(*C)]
    assert box.take([A[2]]) is None


def test_settle_splits_a_mixed_report_between_its_owners():
    from webdgs_amd.ops import CapacityReports, Overflow
    box, report = CapacityReports(), _capacity(A, B, C)
    got = box.settle(OWN, _raises(report))
    assert got.mine == [Overflow(*A), Overflow(*C)] and got.foreign is True and got.error is report
    assert len(box.pending) == 1 and CapacityReports.parse(box.pending[0]) == [Overflow(*B)]
    assert box.take(OWN) is None
    left = box.take([B[2]])
    assert left is not None and CapacityReports.parse(left) == [Overflow(*B)] and box.pending == []


def test_settle_sorts_a_pending_report_by_the_same_rule():
    from webdgs_amd.ops import CapacityReports, Overflow
    box, report = CapacityReports(), _capacity(B, A)
    box.post(report)
    got = box.settle(OWN, _raises(None))
    assert got.mine == [Overflow(*A)] and got.foreign is True and got.error is report
    assert [CapacityReports.parse(e) for e in box.pending] == [[Overflow(*B)]]
    # ... also behind a wait whose own report had no line of ours: both others' lines wait for their owners
    box = CapacityReports()
    box.post(report)
    got = box.settle(OWN, _raises(_capacity(PASSES[3])))
    assert got.mine == [Overflow(*A)] and got.foreign is True and got.error is report
    assert [CapacityReports.parse(e) for e in box.pending] == [[Overflow(*PASSES[3])], [Overflow(*B)]]


def test_settle_lets_the_skipped_step_and_other_errors_through():
    from webdgs_amd.ops import CapacityError, CapacityReports, WdgsError
    box, waiting = CapacityReports(), _capacity(A)
    box.post(waiting)
    skipped = CapacityError(-3, SKIPPED[len("[wdgs -3] "):])
    with pytest.raises(CapacityError) as caught:
        box.settle(OWN, _raises(skipped))
    assert caught.value is skipped and box.pending == [waiting], "nobody's report: raised unchanged, the mailbox untouched"
    other = WdgsError(-1, "wdgs_buffer_create: size must be positive")
    with pytest.raises(WdgsError) as caught:
        box.settle(OWN, _raises(other))
    assert caught.value is other and box.pending == [waiting]
    with pytest.raises(KeyError):
        box.settle(OWN, _raises(KeyError("not the library's")))


@pytest.mark.parametrize("args,want", GROWN)
def test_grown_tile_entries(args, want):
    from webdgs_amd.ops import grownTileEntries
    assert grownTileEntries(*args) == want


def test_the_node_host_settles_and_grows_the_same():
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not available")
    src = """
      const { CapacityReports, grownTileEntries } = require(process.argv[1]);
      const [A, B, C, D] = JSON.parse(process.argv[2]).map((p) => ({ needed: p[0], capacity: p[1], handle: BigInt(p[2]) }));
      const line = (p) => `${p.needed} entries needed, max_tile_entries = ${p.capacity} (forward pass 0x${p.handle.toString(16)})`;
      const capacity = (...ps) => Object.assign(new Error('[wdgs -3] tile entries overflow: ' + ps.map(line).join('; ') + ' (raise wdgs_tiled_forward_config.max_tile_entries)'), { code: 'WDGS_E_CAPACITY' });
      const raises = (e) => () => { if (e) throw e; };
      const same = (got, want) => got.length === want.length && got.every((o, i) => o.needed === want[i].needed && o.capacity === want[i].capacity && o.handle === want[i].handle);
      const parsed = (box) => box.pending.map((e) => CapacityReports.parse(e));
      const thrown = (f) => { try { f(); } catch (e) { return e; } return null; };
      const own = [A.handle, C.handle], out = {};
      let box = new CapacityReports(), got = box.settle(own, raises(null));
      out.nothing = got.mine.length === 0 && got.foreign === false && got.error === null && box.pending.length === 0;
      let report = capacity(C, A); box = new CapacityReports(); got = box.settle(own, raises(report));
      out.own = same(got.mine, [C, A]) && got.foreign === false && got.error === report && box.pending.length === 0;
      box = new CapacityReports(); got = box.settle([A.handle], raises(capacity(B, C)));
      out.others = got.mine.length === 0 && got.foreign === true && got.error === null && box.pending.length === 1 && same(parsed(box)[0], [B, C]) && box.take([A.handle]) === null;
      report = capacity(A, B, C); box = new CapacityReports(); got = box.settle(own, raises(report));
      out.mixed = same(got.mine, [A, C]) && got.foreign === true && got.error === report && box.pending.length === 1 && same(parsed(box)[0], [B]) && box.take(own) === null;
      const left = box.take([B.handle]);
      out.mixedLeft = left !== null && left.code === 'WDGS_E_CAPACITY' && same(CapacityReports.parse(left), [B]) && box.pending.length === 0;
      report = capacity(B, A); box = new CapacityReports(); box.post(report); got = box.settle(own, raises(null));
      out.pending = same(got.mine, [A]) && got.foreign === true && got.error === report && box.pending.length === 1 && same(parsed(box)[0], [B]);
      box = new CapacityReports(); box.post(report); got = box.settle(own, raises(capacity(D)));
      out.pendingBehindOthers = same(got.mine, [A]) && got.error === report && box.pending.length === 2 && same(parsed(box)[0], [D]) && same(parsed(box)[1], [B]);
      const waiting = capacity(A), skipped = Object.assign(new Error(process.argv[3]), { code: 'WDGS_E_CAPACITY' }), other = Object.assign(new Error('[wdgs -1] wdgs_buffer_create: size must be positive'), { code: 'WDGS_E' });
      box = new CapacityReports(); box.post(waiting);
      out.skipped = thrown(() => box.settle(own, raises(skipped))) === skipped && box.pending.length === 1 && box.pending[0] === waiting;
      out.other = thrown(() => box.settle(own, raises(other))) === other && box.pending.length === 1 && box.pending[0] === waiting;
      out.grown = JSON.parse(process.argv[4]).map((g) => grownTileEntries(g[0][0], g[0][1]) === g[1]);
      console.log(JSON.stringify(out));
    """
    r = subprocess.run([node, "-e", src, REPORTS_JS, json.dumps([[n, c, hex(h)] for n, c, h in PASSES]), SKIPPED, json.dumps(GROWN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == dict(nothing=True, own=True, others=True, mixed=True, mixedLeft=True, pending=True, pendingBehindOthers=True,
                                                                 skipped=True, other=True, grown=[True] * 4)


# ---- the pass sets of the trainer (trainer.PassSet), without a device: stub ops that record their destroy()
def test_destroying_pass_sets_destroys_every_op_once_in_set_order():
    from webdgs_amd.trainer import PassSet, destroy_pass_sets
    log = []

    class Stub:
        def __init__(self, name):
            self.name = name

        def destroy(self):
            log.append(self.name)

    shared_camera = Stub("camera of the trainer")
    sets = [PassSet(Stub("t0.fw"), Stub("t0.rast"), Stub("t0.bw")), PassSet(Stub("t1.fw"), Stub("t1.rast"), Stub("t1.bw")),
            PassSet(Stub("m0.fw"), Stub("m0.rast"), Stub("m0.metric"), target=Stub("m0.target"), cameraBuffer=shared_camera),
            PassSet(Stub("m1.fw"), Stub("m1.rast"), Stub("m1.metric"), target=Stub("m1.target"), cameraBuffer=Stub("m1.camera"), ownsCamera=True),
            PassSet(Stub("e0.fw"), Stub("e0.rast"))]
    destroy_pass_sets(sets)
    assert log == ["t0.fw", "t0.rast", "t0.bw", "t1.fw", "t1.rast", "t1.bw", "m0.fw", "m0.rast", "m0.metric", "m0.target",
                   "m1.fw", "m1.rast", "m1.metric", "m1.target", "m1.camera", "e0.fw", "e0.rast"]
    assert "camera of the trainer" not in log, "metric set 0 renders through the trainer's own camera block, which outlives it"
