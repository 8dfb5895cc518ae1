'use strict';
// Developer tool: cube.rolling / cube.shift (one device call for the stored measures, HipStore.rollingMany ->
// olap_store_rolling_multi) against the definition run as written by the same build (Cube._rollingPerItem: one
// dice -> drillUp chain per item of the dimension and a host assembly), in the same process, in alternating rounds (the
// two paths also take turns at going first); medians of the whole call, ended by reading one cell of every measure.
//   [100, 100, 12] along each of its dimensions and a [100, 36 months, 100] cube along time, with 1 and 8 Float32
//   measures; windows: trailing 3, trailing 12 within the year, a lag of 1.
// Usage: node tools/rolling_bench.js [out.txt]      ROLLING_BENCH_ROUNDS=n overrides the rounds of every case
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
const months = () => {
  const d = generic([100, 1, 100]);
  d[1] = new TimeDimension('time', 'month', '2010-01', '2012-12');
  return d;
};

const CASES = [];
for (const measures of [1, 8]) {
  for (const over of [0, 1, 2]) CASES.push({ label: '[100, 100, 12]', dims: () => generic([100, 100, 12]), measures, id: `d${over}`, window: [2, 0], attribute: 'all', rounds: 3 });
  CASES.push({ label: '[100, 100, 12]', dims: () => generic([100, 100, 12]), measures, id: 'd2', window: [1, -1], attribute: 'all', rounds: 3 });
  CASES.push({ label: '[100, 36 months, 100]', dims: months, measures, id: 'time', window: [2, 0], attribute: 'all', rounds: 3 });
  CASES.push({ label: '[100, 36 months, 100]', dims: months, measures, id: 'time', window: [11, 0], attribute: 'year', rounds: 3 });
  CASES.push({ label: '[100, 36 months, 100]', dims: months, measures, id: 'time', window: [12, -12], attribute: 'all', rounds: 3 });
}

say(`# node ${process.version}`);
say(`${'cube'.padStart(22)} ${'measures'.padStart(8)} ${'rolling'.padStart(26)} ${'items'.padStart(6)} ${'rounds'.padStart(6)} | ${'per item'.padStart(11)} ${'one call'.padStart(11)} ${'launches'.padStart(8)} ${'ratio'.padStart(8)}`);
for (const { label, dims, measures, id, window, attribute, rounds: planned } of CASES) {
  const rounds = process.env.ROLLING_BENCH_ROUNDS ? Number(process.env.ROLLING_BENCH_ROUNDS) : planned;
  const cube = fill(new Cube(dims()), measures);
  const ids = cube.storedMeasureIds;
  let checksum = 0;
  let launches = null;
  const once = (device) => {
    const us = clock(() => {
      const out = device ? cube.rolling(id, window[0], window[1], attribute) : cube._rollingPerItem(id, window[0], window[1], attribute);
      if (device) launches = HipStore.lastBatchLaunches;
      for (const m of ids) checksum += out.storedMeasures[m].getValue(cube.storeSize - 1); // waits for the device
    });
    if (device && HipStore.lastRollingPath !== 'device') throw new Error('the device path did not run');
    return us;
  };
  once(true);
  once(false);
  const chain = [];
  const call = [];
  for (let r = 0; r < rounds; ++r) {
    for (const device of r % 2 ? [true, false] : [false, true]) (device ? call : chain).push(once(device));
  }
  const l = median(chain);
  const p = median(call);
  say(`${label.padStart(22)} ${String(measures).padStart(8)} ${`${id} (${window}) by ${attribute}`.padStart(26)} ${String(cube.getDimension(id).numItems).padStart(6)} ${String(rounds).padStart(6)} | ${fmt(l)} ${fmt(p)} ${String(launches).padStart(8)} ${((l / p).toFixed(1) + 'x').padStart(8)}`);
  if (Number.isNaN(checksum)) throw new Error('the results were not read');
}
