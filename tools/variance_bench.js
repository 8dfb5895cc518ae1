'use strict';
// Developer tool: cube.variance (one device call for the stored measures, HipStore.varianceMany ->
// olap_store_variance_multi) against the definition written out on the host by the same build (Cube._varianceHost:
// getData, two folds per output cell in JavaScript, setData), in the same process, in alternating rounds (the two paths
// also take turns at going first); medians of the whole call, ended by reading one cell of every measure.
//   [100, 100, 12] along each of its dimensions by 'all', a [100, 36 months, 100] cube along time by 'year', and a
//   [10, 730 days, 100] cube along time by 'month', with 1 and 8 Float32 measures (the shapes of tools/quantile_bench.js).
// Usage: node tools/variance_bench.js [out.txt]      VARIANCE_BENCH_ROUNDS=n overrides the rounds of every case
const fs = require('fs');
const { Cube, GenericDimension, TimeDimension, HipStore } = require('../olap-in-memory_amd/js');

const lines = [];
const say = (s) => {
  console.log(s);
  lines.push(s);
  if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
};
const median = (t) => t.slice().sort((a, b) => a - b)[Math.floor(t.length / 2)];
const clock = (fn) => {
  const t0 = process.hrtime.bigint();
  fn();
  return Number(process.hrtime.bigint() - t0) / 1e3;
};
const fmt = (us) => (us >= 1e4 ? `${(us / 1e3).toFixed(2)} ms` : `${us.toFixed(1)} us`).padStart(11);

function fill(cube, measures) {
  const n = cube.storeSize;
  for (let k = 0; k < measures; ++k) {
    cube.createStoredMeasure(`m${k}`, {}, 'float32', 0);
    const values = new Float32Array(n);
    for (let i = 0; i < n; ++i) values[i] = ((i * (k + 3)) % 17) * 0.25; // 0 (unset) in one cell of 17
    cube.setData(`m${k}`, values);
  }
  return cube;
}
const generic = (lens) => lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
const withTime = (lens, root, from, to) => {
  const d = generic(lens);
  d[1] = new TimeDimension('time', root, from, to);
  return d;
};

const CASES = [];
for (const measures of [1, 8]) {
  for (const over of [0, 1, 2]) CASES.push({ label: '[100, 100, 12]', dims: () => generic([100, 100, 12]), measures, id: `d${over}`, attribute: 'all', rounds: 5 });
  CASES.push({ label: '[100, 36 months, 100]', dims: () => withTime([100, 1, 100], 'month', '2010-01', '2012-12'), measures, id: 'time', attribute: 'year', rounds: 5 });
  CASES.push({ label: '[10, 730 days, 100]', dims: () => withTime([10, 1, 100], 'day', '2010-01-01', '2011-12-31'), measures, id: 'time', attribute: 'month', rounds: 5 });
}

say(`# node ${process.version}`);
say(`${'cube'.padStart(22)} ${'measures'.padStart(8)} ${'stddev, ddof 1'.padStart(18)} ${'items'.padStart(6)} ${'rounds'.padStart(6)} | ${'on the host'.padStart(11)} ${'one call'.padStart(11)} ${'launches'.padStart(8)} ${'ratio'.padStart(8)}`);
for (const { label, dims, measures, id, attribute, rounds: planned } of CASES) {
  const rounds = process.env.VARIANCE_BENCH_ROUNDS ? Number(process.env.VARIANCE_BENCH_ROUNDS) : planned;
  const cube = fill(new Cube(dims()), measures);
  const ids = cube.storedMeasureIds;
  let checksum = 0;
  let launches = null;
  const once = (device) => {
    const us = clock(() => {
      const out = device ? cube.stddev(id, attribute, 1) : cube._varianceHost(id, attribute, 1, 1);
      if (device) launches = HipStore.lastBatchLaunches;
      for (const m of ids) checksum += out.storedMeasures[m].getValue(out.storeSize - 1); // waits for the device
    });
    if (device && HipStore.lastVariancePath !== 'device') throw new Error('the device path did not run');
    return us;
  };
  once(true);
  once(false);
  const host = [];
  const call = [];
  for (let r = 0; r < rounds; ++r) {
    for (const device of r % 2 ? [true, false] : [false, true]) (device ? call : host).push(once(device));
  }
  const l = median(host);
  const p = median(call);
  say(`${label.padStart(22)} ${String(measures).padStart(8)} ${`${id} by ${attribute}`.padStart(18)} ${String(cube.getDimension(id).numItems).padStart(6)} ${String(rounds).padStart(6)} | ${fmt(l)} ${fmt(p)} ${String(launches).padStart(8)} ${((l / p).toFixed(1) + 'x').padStart(8)}`);
  if (Number.isNaN(checksum)) throw new Error('the results were not read');
}
