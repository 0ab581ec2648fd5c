// Typings of capacity_reports.js: who answers a truncated tile-entry list, and by how much the lists grow (no addon needed to load it).
/** One pass's line of a capacity report: the entries its frame needed, what its lists hold, the forward pass's handle. */
export interface Overflow { needed: number; capacity: number; handle: bigint; }
/** What settle() found for one owner: its passes' lines, whether a line was left for another owner, the report its lines came from (null: none). */
export interface Settled { mine: Overflow[]; foreign: boolean; error: Error | null; }
/** Tile-entry lists after an overflow: min(max(2 * now, floor(needed * 1.5)), 0xFFFFF000). */
export function grownTileEntries(now: number, needed: number): number;
/** Capacity reports that reached the wrong owner (a Trainer, its Evaluator and a Viewer sharing a device): left here for the owner of the passes they name. */
export class CapacityReports {
  constructor(keep?: number);
  pending: Error[];
  /** wait(), then the WDGS_E_CAPACITY report it threw (or the oldest pending one that names an own pass) sorted by the one rule: own lines are
   *  returned, the other owners' lines posted as a report of their own.  A report that names no pass and every other error propagate. */
  settle(ownHandles: Array<bigint | number>, wait: () => void): Settled;
  /** One record per pass a capacity report names (csrc/api.hip: deferred_checks, wdgs_tiled_forward_check), in its order; [] for any other error. */
  static parse(error: Error): Overflow[];
  /** The records about `ownHandles`' passes, and whether the report also names passes of another owner. */
  static split(error: Error, ownHandles: Array<bigint | number>): { mine: Overflow[]; others: boolean };
  static passesNamed(error: Error): bigint[];
  post(error: Error): void;
  take(ownHandles: Array<bigint | number>): Error | null;
}
