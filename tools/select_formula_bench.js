'use strict';
// Developer tool: getTotalForDimensionItems / copyMeasureData of a computed measure (the two-input Float32 formula
// `uu * vv + 1`) on the device (HipStore.selectTotalFormula / copySelectFormula: one launch over the selection)
// against the per-cell path (getSingleData: one blocking getValue per input per combination, plus a setValue per
// copied cell), empty filter, at 10^4, 10^5 and 10^6 combinations.  The per-cell side runs at 10^4 and 10^5 only.
// Usage: node tools/select_formula_bench.js [out.txt]
const fs = require('fs');
const { Cube, GenericDimension, HipStore } = require('../olap-in-memory_amd/js');

const lines = [];
const say = (s) => {
  console.log(s);
  lines.push(s);
};
const time = (fn, reps) => {
  fn();
  const t = [];
  for (let i = 0; i < reps; ++i) {
    const t0 = process.hrtime.bigint();
    fn();
    t.push(Number(process.hrtime.bigint() - t0) / 1e3);
  }
  t.sort((a, b) => a - b);
  return t[Math.floor(t.length / 2)];
};
const fmt = (us) => (us === null ? 'skipped'.padStart(12) : (us >= 1e4 ? `${(us / 1e3).toFixed(1)} ms` : `${us.toFixed(1)} us`).padStart(12));

say(`${'combos'.padStart(8)} ${'total dev'.padStart(12)} ${'path'.padStart(10)} ${'total/cell'.padStart(12)} ${'copy dev'.padStart(12)} ${'copy path'.padStart(10)} ${'copy/cell'.padStart(12)}`);
for (const lens of [[100, 100], [100, 1000], [1000, 1000]]) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  cube.createStoredMeasure('uu', {}, 'float32', 0);
  cube.createStoredMeasure('vv', {}, 'float32', 0);
  cube.createStoredMeasure('tt', {}, 'float32', 0);
  const n = cube.storeSize;
  cube.setData('uu', Float32Array.from({ length: n }, (_, i) => (i % 97) * 0.5));
  cube.setData('vv', Float32Array.from({ length: n }, (_, i) => 1 + (i % 13)));
  cube.createComputedMeasure('ww', 'uu * vv + 1');
  HipStore.lastSelectPath = null;
  HipStore.lastCopyPath = null;
  const dev = time(() => cube.getTotalForDimensionItems('ww', {}), 50);
  const path = HipStore.lastSelectPath;
  const copy = time(() => cube.copyMeasureData('ww', 'tt', {}), 50);
  const copyPath = HipStore.lastCopyPath;
  const perCell = n <= 1e5 ? time(() => cube._getTotalForDimensionItemsPerCell('ww', {}), 1) : null;
  const copyCell = n <= 1e5 ? time(() => cube._copyMeasureDataPerCell('ww', 'tt', {}), 1) : null;
  say(`${String(n).padStart(8)} ${fmt(dev)} ${String(path).padStart(10)} ${fmt(perCell)} ${fmt(copy)} ${String(copyPath).padStart(10)} ${fmt(copyCell)}`);
}
if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
