'use strict';
/*
 * capacity_reports.js (+ capacity_reports.d.ts) -- who answers a truncated tile-entry list, and by how much the lists grow.  Plain JavaScript with no
 * require of the N-API addon, so it loads (and is tested) where the HIP runtime is missing; webdgs_hip.js re-exports it under the same names.
 * webdgs_amd/ops.py holds the twin: CapacityReports, Settled, grownTileEntries.
 */

/** Tile-entry lists after an overflow: twice what they hold, or 1.5 x what the frame needed where that is more; never more than a sort takes. */
function grownTileEntries(now, needed) { return Math.min(Math.max(2 * now, Math.floor(needed * 1.5)), 0xFFFFF000); }

/** Capacity reports that reached the wrong owner.  The library reports a truncated tile-entry list at the next host wait on the DEVICE, to whoever waits
 *  (csrc/api.hip: deferred_checks consumes every pass's word and names up to four passes).  The owners of forward passes on a device -- a Trainer's
 *  training and metric sets, its Evaluator's sets, a Viewer -- all wait through settle(), which has the one rule: an owner keeps the lines about its own
 *  passes, every other line is left here as a report of its own, where the passes' owner finds it at its own next wait. */
class CapacityReports {
  constructor(keep) { this.pending = []; this.keep = keep || 16; }
  /** wait(), then the capacity report it threw -- or, if that had no line of `ownHandles`' passes, the oldest pending report that has one -- sorted:
   *  { mine, foreign, error } -- the owner's lines, whether a line was left for another owner, the report the owner's lines came from (null when there
   *  are none).  A report that names no pass (an optimizer step skipped on every rank: nobody's) and every other error propagate. */
  settle(ownHandles, wait) {
    let mine = [], foreign = false, report = null;
    try { wait(); } catch (e) {
      if (!(e && e.code === 'WDGS_E_CAPACITY') || !CapacityReports.parse(e).length) throw e;
      report = e;
      ({ mine, others: foreign } = this.keepOwn(report, ownHandles));
    }
    if (!mine.length) {
      report = this.take(ownHandles);
      if (report) { const kept = this.keepOwn(report, ownHandles); mine = kept.mine; foreign = foreign || kept.others; }
    }
    return { mine, foreign, error: mine.length ? report : null };
  }
  /** split(); the other owners' lines are posted as one report in deferred_checks' format, so that parse() stays the reader of report text. */
  keepOwn(report, ownHandles) {
    const { mine, others } = CapacityReports.split(report, ownHandles);
    if (others) {
      const lines = CapacityReports.parse(report).filter((o) => !mine.some((m) => m.handle === o.handle))
        .map((o) => `${o.needed} entries needed, max_tile_entries = ${o.capacity} (forward pass 0x${o.handle.toString(16)})`).join('; ');
      this.post(Object.assign(new Error(`[wdgs -3] tile entries overflow: ${lines} (raise wdgs_tiled_forward_config.max_tile_entries)`), { code: 'WDGS_E_CAPACITY' }));
    }
    return { mine, others };
  }
  /** [{ needed, capacity, handle }] -- one record per pass the report names, in the report's order (handle: a BigInt); [] for any other error.  The one
   *  reader of report text (webdgs_amd/ops.py has its twin).  It follows two format strings of csrc/api.hip:
   *    deferred_checks:          "tile entries overflow: " + "%u entries needed, max_tile_entries = %u (forward pass %p)" joined by "; " + " (raise ...)"
   *    wdgs_tiled_forward_check: "tile entries overflow: %u entries needed, max_tile_entries = %u (forward pass %p)"
   *  Known limit: the library names at most four passes per report; a fifth that overflowed in the same wait is consumed unnamed. */
  static parse(error) {
    const out = [], re = /(\d+) entries needed, max_tile_entries = (\d+) \(forward pass (0x[0-9a-fA-F]+)\)/g, text = String(error && error.message);
    for (let m = re.exec(text); m; m = re.exec(text)) out.push({ needed: Number(m[1]), capacity: Number(m[2]), handle: BigInt(m[3]) });
    return out;
  }
  /** { mine, others }: the records about `ownHandles`' passes, and whether the report also names passes of another owner. */
  static split(error, ownHandles) {
    const own = ownHandles.map((h) => BigInt(h)), named = CapacityReports.parse(error);
    const mine = named.filter((o) => own.some((h) => h === o.handle));
    return { mine, others: mine.length < named.length };
  }
  static passesNamed(error) { return CapacityReports.parse(error).map((o) => o.handle); }
  post(error) { this.pending.push(error); if (this.pending.length > this.keep) this.pending.splice(0, this.pending.length - this.keep); }
  /** The oldest pending report that names one of `ownHandles` (removed), or null. */
  take(ownHandles) {
    for (let i = 0; i < this.pending.length; i++) {
      if (CapacityReports.split(this.pending[i], ownHandles).mine.length) return this.pending.splice(i, 1)[0];
    }
    return null;
  }
}

module.exports = { CapacityReports, grownTileEntries };
