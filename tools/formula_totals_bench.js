'use strict';
// Developer tool: getNestedObjects(['ww'], true) of a computed measure over 1, 2 and 4 Float32 inputs on the device path
// (HipStore.totalsFormula: the inputs' extended cubes built and the formula evaluated on the device, one copy) against
// the chain of drillUps (Cube._getNestedObjectsChain: 2^D - 1 cube roll-ups, 2^D evaluations and merges) in the same
// process, in alternating rounds; the cube holds 4 stored measures.  `call` is the device call alone and `object` the
// host's toNestedObject over its result: the two halves of the device path.
// Usage: node tools/formula_totals_bench.js [out.txt]
const fs = require('fs');
const { Cube, GenericDimension, HipStore } = require('../olap-in-memory_amd/js');
const { toNestedObject } = require('../olap-in-memory_amd/js/formatter');

const lines = [];
const say = (s) => {
  console.log(s);
  lines.push(s);
};
const median = (t) => t.slice().sort((a, b) => a - b)[Math.floor(t.length / 2)];
const clock = (fn) => {
  const t0 = process.hrtime.bigint();
  fn();
  return Number(process.hrtime.bigint() - t0) / 1e3;
};
const fmt = (us) => (us >= 1e4 ? `${(us / 1e3).toFixed(1)} ms` : `${us.toFixed(1)} us`).padStart(12);
const FORMULA = { 1: 'aa * 3 + 1', 2: 'aa * bb + 1', 4: 'aa * bb + cc - dd' };

say(`${'shape'.padStart(16)} ${'E cells'.padStart(9)} ${'inputs'.padStart(6)} ${'device'.padStart(12)} ${'call'.padStart(12)} ${'object'.padStart(12)} ${'chain'.padStart(12)} ${'path'.padStart(8)} ${'launches'.padStart(8)}`);
for (const lens of [[3, 2], [10, 10, 10], [12, 50, 20], [10, 10, 10, 10], [10, 10, 10, 10, 10, 10]]) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  const n = cube.storeSize;
  ['aa', 'bb', 'cc', 'dd'].forEach((id, k) => {
    cube.createStoredMeasure(id, {}, 'float32', 0);
    cube.setData(id, Float32Array.from({ length: n }, (_, i) => ((i * (k + 3)) % 17) * 0.25));
  });
  const ext = lens.reduce((p, l) => p * (l + 1), 1);
  const extended = cube.dimensions.map((d) => ({ getItems: () => d.getItems().concat(['all']) }));
  const rounds = n >= 1e6 ? 3 : n >= 1e4 ? 7 : 21;
  for (const inputs of [1, 2, 4]) {
    cube.createComputedMeasure('ww', FORMULA[inputs]);
    const f = cube._totalsFormula('ww');
    const rules = f.ids.map(() => cube.dimensions.map(() => undefined));
    const t = { device: [], call: [], object: [], chain: [] };
    HipStore.lastTotalsPath = null;
    for (let r = -1; r < rounds; ++r) { // (round -1 warms both sides up)
      const device = clock(() => cube.getNestedObjects(['ww'], true));
      const chain = clock(() => cube._getNestedObjectsChain(['ww']));
      let values;
      const call = clock(() => {
        values = HipStore.totalsFormula(f.program, f.stores, cube.dimensions, rules);
      });
      const object = clock(() => toNestedObject(values, extended));
      if (r >= 0) {
        t.device.push(device);
        t.chain.push(chain);
        t.call.push(call);
        t.object.push(object);
      }
    }
    say(`${`[${lens.join(',')}]`.padStart(16)} ${String(ext).padStart(9)} ${String(inputs).padStart(6)} ${fmt(median(t.device))} ${fmt(median(t.call))} ${fmt(median(t.object))} ${fmt(median(t.chain))} ${String(HipStore.lastTotalsPath).padStart(8)} ${String(HipStore.lastTotalsLaunches).padStart(8)}`);
    cube.dropMeasure('ww');
  }
}
if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
