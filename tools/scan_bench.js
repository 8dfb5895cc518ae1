'use strict';
// Developer tool: cube.iterateOverDimension / cube.scan with a callback that reads getData of every measure, through the
// one device pass (HipStore.blocksMany -> olap_store_blocks_report, then host-resident stores) and through the
// per-combination loop of the same build (Cube._iterateOverDimensionPerCombination / _scanPerCombination: a dice, a fused
// dice -> drillUp per measure group and a device-to-host copy per combination), in the same process, in alternating
// rounds (the two paths also take turns at going first); medians of the whole call.
//   [100, 100, 12] iterated over each of its dimensions with 1, 4 and 8 Float32 measures: many small blocks;
//   scans with few combinations of large blocks: where the line to the per-combination path would have to be drawn.
// Usage: node tools/scan_bench.js [out.txt]      SCAN_BENCH_ROUNDS=n overrides the rounds of every case
const fs = require('fs');
const { Cube, GenericDimension, HipStore } = require('../olap-in-memory_amd/js');

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

function build(lens, measures) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  const n = cube.storeSize;
  for (let k = 0; k < measures; ++k) {
    cube.createStoredMeasure(`m${k}`, {}, 'float32', 0);
    const values = new Float32Array(n);
    for (let i = 0; i < n; ++i) values[i] = ((i * (k + 3)) % 17) * 0.25; // 0 (unset) in one cell of 17
    cube.setData(`m${k}`, values);
  }
  return cube;
}

const CASES = [];
for (const measures of [1, 4, 8]) for (const over of [0, 1, 2]) CASES.push({ lens: [100, 100, 12], measures, method: 'iterateOverDimension', arg: `d${over}`, rounds: over === 2 ? 3 : 5 });
// few combinations of large blocks
for (const measures of [1, 4]) {
  CASES.push({ lens: [256, 100, 100], measures, method: 'scan', arg: ['d0'], rounds: 5 }); // 10^4 cells per combination
  CASES.push({ lens: [32, 1000, 100], measures, method: 'scan', arg: ['d0'], rounds: 5 }); // 10^5
  CASES.push({ lens: [4, 1000, 1000], measures, method: 'scan', arg: ['d0'], rounds: 5 }); // 10^6
  CASES.push({ lens: [1000, 1000, 4], measures, method: 'scan', arg: ['d2'], rounds: 5 }); // 10^6, transposed
}

say(`# node ${process.version}`);
say(`${'lens'.padStart(16)} ${'measures'.padStart(8)} ${'call'.padStart(28)} ${'combinations'.padStart(12)} ${'rounds'.padStart(6)} | ${'per combination'.padStart(15)} ${'one pass'.padStart(11)} ${'ratio'.padStart(8)}`);
const slower = [];
HipStore.blocksMaxBlockCells = Infinity; // measure both paths on either side of the routing line
for (const { lens, measures, method, arg, rounds: planned } of CASES) {
  const rounds = process.env.SCAN_BENCH_ROUNDS ? Number(process.env.SCAN_BENCH_ROUNDS) : planned;
  const cube = build(lens, measures);
  const ids = cube.storedMeasureIds;
  let combinations = 0;
  let checksum = 0;
  const cb = (handed) => {
    ++combinations;
    for (const id of ids) checksum += handed.getData(id).length;
  };
  const once = (onePass) => {
    combinations = 0;
    const us = clock(() => cube[onePass ? method : `_${method}PerCombination`](arg, cb));
    if (onePass && HipStore.lastBlocksCalls !== 1) throw new Error('the one-pass path did not run');
    return us;
  };
  once(true);
  once(false);
  const loop = [];
  const pass = [];
  for (let r = 0; r < rounds; ++r) {
    for (const onePass of r % 2 ? [true, false] : [false, true]) (onePass ? pass : loop).push(once(onePass));
  }
  const l = median(loop);
  const p = median(pass);
  const call = `${method}(${JSON.stringify(arg)})`;
  if (p > l) slower.push(`${JSON.stringify(lens)} x ${measures} ${call}`);
  say(`${JSON.stringify(lens).padStart(16)} ${String(measures).padStart(8)} ${call.padStart(28)} ${String(combinations).padStart(12)} ${String(rounds).padStart(6)} | ${fmt(l).padStart(15)} ${fmt(p)} ${((l / p).toFixed(1) + 'x').padStart(8)}`);
  if (checksum === 0) throw new Error('the callback read nothing');
}
say(slower.length ? `# the one-pass path is SLOWER than the per-combination loop at: ${slower.join('; ')}` : '# the one-pass path is not slower than the per-combination loop at any measured case');
