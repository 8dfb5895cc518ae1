'use strict';
// Developer tool: Cube.compose (each source cube reshaped once, its measures in one device pass: HipStore.composeMany ->
// olap_store_compose_multi) against Cube._composePerMeasure of the same build (the reference's order of calls: create,
// fill, hydrate, measure by measure), in the same process, in alternating rounds (the two paths also take turns at going
// first); medians of the whole call, closed by reading one cell of every measure of the result so that queued device
// work is included.
//   the reference benchmark's shape (test/cube-benchmark.js:122): 4^10 cells, Float32 measures, a 10 % cube composed
//   with a 50 % cube, with 3 measures per cube as there and with 1 and 8;
//   a union of two 10^7-cell cubes whose first dimension overlaps by half (1.5 * 10^7 cells), with and without fillWith,
//   next to a device-to-device copy of the same measures on the same box (clone(): bytes in + bytes out like the pass).
// Usage: node tools/compose_bench.js [out.txt]      COMPOSE_BENCH_ROUNDS=n overrides the rounds of every case
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
const finish = (cube) => {
  for (const id of cube.storedMeasureIds) cube.storedMeasures[id].getValue(0);
  return cube;
};

// `fill` of the cells hold 1, the others are unset (test/helpers/create-large-test-cube.js:31-46; seeded here)
function cube(dims, prefix, measures, fill) {
  const c = new Cube(dims);
  const n = c.storeSize;
  const values = new Float32Array(n);
  let s = 20240807;
  let left = Math.round(fill * n);
  if (fill >= 1) values.fill(1);
  while (fill < 1 && left > 0) {
    s = (Math.imul(s, 1664525) + 1013904223) | 0;
    const i = (s >>> 0) % n;
    if (values[i] === 0) {
      values[i] = 1;
      --left;
    }
  }
  for (let m = 0; m < measures; ++m) {
    c.createStoredMeasure(`${prefix}${m}`, {}, 'float32', 0);
    c.setData(`${prefix}${m}`, values);
  }
  return c;
}
const items = (d, from, to) => Array.from({ length: to - from }, (_x, j) => `dimension${d}-item${from + j}`);
const dimension = (d, from, to) => new GenericDimension(`dimension${d}`, 'root', items(d, from, to));

const CASES = [];
for (const measures of [3, 1, 8]) {
  CASES.push({
    name: `4^10, ${measures} + ${measures} measures, 10 % o 50 %`,
    build: () => {
      const dims = Array.from({ length: 10 }, (_x, d) => dimension(d, 0, 4));
      return [cube(dims, 'left', measures, 0.1), cube(dims, 'right', measures, 0.5)];
    },
    union: false,
    fillWith: null,
    rounds: 7,
  });
}
for (const filled of [false, true]) {
  CASES.push({
    name: `union of two 10^7-cell cubes, 3 + 3 measures${filled ? ', fillWith' : ''}`,
    build: () => [cube([dimension(0, 0, 100), dimension(1, 0, 1000), dimension(2, 0, 100)], 'left', 3, 0.5),
                  cube([dimension(0, 50, 150), dimension(1, 0, 1000), dimension(2, 0, 100)], 'right', 3, 0.5)],
    union: true,
    fillWith: filled ? { left0: 7, left1: 7, left2: 7, right0: 7, right1: 7, right2: 7 } : null,
    rounds: 5,
    copy: true,
  });
}

say(`# node ${process.version}`);
say(`${'case'.padEnd(58)} ${'cells'.padStart(9)} ${'rounds'.padStart(6)} | ${'per measure'.padStart(11)} ${'launches'.padStart(8)} | ${'one pass'.padStart(11)} ${'launches'.padStart(8)} ${'calls'.padStart(5)} | ${'ratio'.padStart(7)}`);
const slower = [];
for (const { name, build, union, fillWith, rounds: planned, copy } of CASES) {
  const rounds = process.env.COMPOSE_BENCH_ROUNDS ? Number(process.env.COMPOSE_BENCH_ROUNDS) : planned;
  const [left, right] = build();
  const launches = [0, 0];
  let result = null;
  const once = (onePass) => {
    const us = clock(() => {
      result = finish(onePass ? left.compose(right, union, fillWith) : left._composePerMeasure(right, union, fillWith));
    });
    if (onePass && HipStore.lastComposeCalls !== 2) throw new Error('the one-pass path did not run');
    if (onePass) launches[1] = HipStore.lastBatchLaunches;
    return us;
  };
  // the launches of the old path: what every hydrateFromCube's loadMany reports, summed
  const realLoadMany = HipStore.loadMany;
  HipStore.loadMany = function counted(...args) {
    const out = realLoadMany.apply(HipStore, args);
    launches[0] += HipStore.lastBatchLaunches;
    return out;
  };
  once(false);
  HipStore.loadMany = realLoadMany;
  once(true);
  const old = [];
  const pass = [];
  for (let r = 0; r < rounds; ++r) {
    for (const onePass of r % 2 ? [true, false] : [false, true]) (onePass ? pass : old).push(once(onePass));
  }
  const o = median(old);
  const p = median(pass);
  if (p > o) slower.push(name);
  say(`${name.padEnd(58)} ${String(result.storeSize).padStart(9)} ${String(rounds).padStart(6)} | ${fmt(o)} ${String(launches[0]).padStart(8)} | ${fmt(p)} ${String(launches[1]).padStart(8)} ${String(HipStore.lastComposeCalls).padStart(5)} | ${((o / p).toFixed(2) + 'x').padStart(7)}`);
  if (copy) {
    // the same bytes in and out as a plain device-to-device copy: every measure of the result cloned, read back one cell
    const stores = result.storedMeasureIds.map((id) => result.storedMeasures[id]);
    const times = [];
    for (let r = 0; r < rounds + 2; ++r) times.push(clock(() => stores.map((store) => store.clone()).forEach((c) => c.getValue(0))));
    const c = median(times.slice(2));
    const bytes = stores.length * result.storeSize * 4;
    say(`${'  clone() of the result\'s measures (device-to-device copy)'.padEnd(58)} ${String(result.storeSize).padStart(9)} ${String(rounds).padStart(6)} | ${fmt(c)}   ${(2 * bytes / c / 1e3).toFixed(0)} GB/s read + written; the one pass takes ${(p / c).toFixed(2)} of it, ${((bytes + stores.length * 1e7 * 4) / p / 1e3).toFixed(0)} GB/s over its own bytes`);
  }
}
say(slower.length ? `# compose is SLOWER than the per-measure path at: ${slower.join('; ')}` : '# compose is not slower than the per-measure path at any measured case');
