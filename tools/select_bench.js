'use strict';
// Developer tool: Cube.getTotalForDimensionItems / copyMeasureData on the device (one launch over the selection)
// against the per-cell path they replace (one blocking getValue / setValue per combination), at 10^4, 10^6 and
// 10^8 Float32 cells.  The per-cell path runs only where its estimate (12 us per read, 24 us per copied cell) stays
// under a minute.  References: collapse() of the same cube, and a dice of the same selection (materialised).
// Usage: node tools/select_bench.js [out.txt]
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

for (const lens of [[10, 10, 100], [100, 100, 100], [100, 1000, 1000]]) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  cube.createStoredMeasure('mm', {}, 'float32', 0);
  cube.createStoredMeasure('tt', {}, 'float32', 0);
  cube.fillData('mm', 1);
  const cells = cube.storeSize;
  const reps = cells >= 1e8 ? 20 : 100;
  say(`# ${cells} cells (${lens.join(' x ')}), Float32; collapse(): ${fmt(time(() => cube.collapse().getData('mm'), reps))}`);
  const filters = {
    '{}': {},
    'outermost one item': { d0: 'd0i1' },
    'innermost one item': { d2: 'd2i7' },
    'two dims, permuted keys': { d2: ['d2i5', 'd2i1'], d0: ['d0i3', 'd0i0'] },
  };
  say(`${'filter'.padEnd(26)} ${'combos'.padStart(10)} ${'total dev'.padStart(12)} ${'path'.padStart(10)} ${'total/cell'.padStart(12)} ${'copy dev'.padStart(12)} ${'copy/cell'.padStart(12)} ${'dice'.padStart(12)}`);
  for (const [name, f] of Object.entries(filters)) {
    const combos = Object.keys(f).reduce((n, k) => n * (typeof f[k] === 'string' ? 1 : f[k].length), 1) * dims.filter((d) => f[d.id] === undefined).reduce((n, d) => n * d.numItems, 1);
    const dev = time(() => cube.getTotalForDimensionItems('mm', f), reps);
    const path = HipStore.lastSelectPath;
    const perCell = combos * 12 < 60e6 ? time(() => cube._getTotalForDimensionItemsPerCell('mm', f), combos > 1e4 ? 1 : 5) : null;
    const copy = time(() => cube.copyMeasureData('mm', 'tt', f), reps);
    const copyCell = combos * 24 < 60e6 ? time(() => cube._copyMeasureDataPerCell('mm', 'tt', f), combos > 1e4 ? 1 : 5) : null;
    let diced = cube;
    for (const [k, v] of Object.entries(f)) diced = diced.dice(k, 'item', typeof v === 'string' ? [v] : v, true);
    const dice = diced === cube ? null : time(() => {
      let c = cube;
      for (const [k, v] of Object.entries(f)) c = c.dice(k, 'item', typeof v === 'string' ? [v] : v, true);
      return c.storedMeasures.mm._native.size; // materialised
    }, reps);
    say(`${name.padEnd(26)} ${String(combos).padStart(10)} ${fmt(dev)} ${path.padStart(10)} ${fmt(perCell)} ${fmt(copy)} ${fmt(copyCell)} ${fmt(dice)}`);
  }
}
if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
