'use strict';
// Developer tool: cube.convertToStoredMeasure('margin' = revenue - cost) through the host path of the same build
// (Cube._copyToStoredMeasureHost: getData -> plain Array -> setData, the whole cube over PCIe twice) and through the device
// path (HipStore.setFormula -> olap_store_set_formula: one launch), in the same process, in alternating rounds (the two
// paths also take turns at going first); medians.
// `method` is the whole Cube method; `call` is the device call alone (addon setFormula into an existing store: the launch
// and its one synchronisation), given with the kernel's algorithmic bytes (inputs read once + cells written once).
// `all ops` is the same call with OLAP_SET_FORMULA_ALL_OPS=1: the instantiation that carries the library routines (pow, sin,
// ...: 222 VGPRs, 2 waves per SIMD) instead of the plain one (40 VGPRs, 8 waves per SIMD), in alternating rounds.
// Usage: node tools/materialize_bench.js [out.txt]
const fs = require('fs');
const v8 = require('v8');
const { Cube, GenericDimension, HipStore } = require('../olap-in-memory_amd/js');

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
const fmt = (us) => (us >= 1e4 ? `${(us / 1e3).toFixed(2)} ms` : `${us.toFixed(1)} us`).padStart(11);

function build(lens, type) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  const n = cube.storeSize;
  const TA = type === 'float64' ? Float64Array : Float32Array;
  ['revenue', 'cost'].forEach((id, k) => {
    cube.createStoredMeasure(id, {}, type, 0);
    const values = new TA(n);
    for (let i = 0; i < n; ++i) values[i] = ((i * (k + 3)) % 17) * 0.25 + k; // revenue - cost is 0 (unset) in about one cell of 17
    cube.setData(id, values);
  });
  return cube;
}

const heapLimit = v8.getHeapStatistics().heap_size_limit;
say(`# node ${process.version}, heap limit ${(heapLimit / 2 ** 30).toFixed(2)} GiB`);
say(`${'cells'.padStart(10)} ${'cell type'.padStart(9)} ${'rounds'.padStart(6)} | ${'method: host'.padStart(12)} ${'device'.padStart(11)} ${'ratio'.padStart(7)} | ${'call: device'.padStart(12)} ${'bytes'.padStart(10)} ${'GB/s'.padStart(8)} | ${'all ops'.padStart(11)} ${'GB/s'.padStart(8)}`);

const CASES = [
  { lens: [100, 100], type: 'float32', rounds: 15 },
  { lens: [100, 100, 100], type: 'float32', rounds: 9 },
  { lens: [100, 100, 100], type: 'float64', rounds: 9 },
  { lens: [1000, 100, 100], type: 'float32', rounds: 5 },
  { lens: [1000, 1000, 100], type: 'float32', rounds: 3 },
];
const slower = [];
for (const { lens, type, rounds } of CASES) {
  const cells = lens.reduce((p, l) => p * l, 1);
  // the host path holds a plain Array (8 bytes per cell on the V8 heap) and a Float64Array of the cube at once
  const hostFits = cells * 8 * 1.5 < heapLimit;
  const cube = build(lens, type);
  const once = (device) => {
    cube.createComputedMeasure('margin', 'revenue - cost');
    const us = clock(() => {
      if (device) cube.convertToStoredMeasure('margin', {}, type, 0);
      else cube._copyToStoredMeasureHost('margin', 'margin', {}, type, 0, true);
    });
    if (device && HipStore.lastMaterializePath !== 'device') throw new Error('the device path did not run');
    cube.dropMeasure('margin');
    return us;
  };
  if (hostFits) once(false);
  once(true);
  const host = [];
  const device = [];
  for (let r = 0; r < rounds; ++r) {
    const order = r % 2 ? [true, false] : [false, true];
    for (const dev of order) {
      if (dev) device.push(once(true));
      else if (hostFits) host.push(once(false));
    }
  }
  // the device call alone, into one existing store
  cube.createStoredMeasure('frozen', {}, type, 0);
  const program = { code: Int32Array.of(1, 0, 1, 1, 4), consts: new Float64Array(0) }; // INPUT 0, INPUT 1, SUB
  const inputs = [cube.storedMeasures.revenue, cube.storedMeasures.cost];
  const call = [];
  const allOps = [];
  for (let r = 0; r < 2 * Math.max(rounds, 7); ++r) {
    const all = (r + (r >> 1)) % 2 === 1; // plain, all, all, plain, ...
    if (all) process.env.OLAP_SET_FORMULA_ALL_OPS = '1';
    (all ? allOps : call).push(clock(() => cube.storedMeasures.frozen.setFormula(program, inputs, [])));
    delete process.env.OLAP_SET_FORMULA_ALL_OPS;
  }
  const bytes = cells * (type === 'float64' ? 8 : 4) * 3;
  const h = hostFits ? median(host) : NaN;
  const d = median(device);
  const c = median(call);
  const a = median(allOps);
  if (hostFits && d > h) slower.push(`${cells} ${type}`);
  say(`${String(cells).padStart(10)} ${type.padStart(9)} ${String(rounds).padStart(6)} | ${(hostFits ? fmt(h) : 'heap'.padStart(11)).padStart(12)} ${fmt(d)} ${(hostFits ? (h / d).toFixed(1) + 'x' : '-').padStart(7)} | ${fmt(c).padStart(12)} ${String(bytes).padStart(10)} ${(bytes / c / 1e3).toFixed(1).padStart(8)} | ${fmt(a)} ${(bytes / a / 1e3).toFixed(1).padStart(8)}`);
}
say(slower.length ? `# the device path is SLOWER than the host path at: ${slower.join('; ')}` : '# the device path is not slower than the host path at any measured size');
say("# 'heap': the host path's plain Array of the cube does not fit this node's heap; only the device path ran");
if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
