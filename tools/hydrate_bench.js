'use strict';
// Developer tool: Cube.hydrateFromSparseNestedObject as one batched setValues against the retained per-cell walk
// (Cube._hydrateFromSparseNestedObjectPerCell: one blocking setValue per leaf), at 10^3, 10^5 and 10^6 leaves on a
// 10^6-cell and a 10^8-cell Float32 cube, for a plain `sum` measure and a tracked `first` one.  Every run starts from a
// fresh measure.  Columns: walk = the host walk alone (setValues stubbed), setValues = HipStore.setValues on the
// walk's lists, native = the addon call on ready Float64Arrays (conversion excluded), batched = the whole call.
// The per-cell walk (about 15 us per leaf) runs up to 10^5 leaves, and at 10^6 leaves once (10^6 cells, sum).
// Usage: node tools/hydrate_bench.js [out.txt]
//        node tools/hydrate_bench.js --native N   (N-entry setValues calls only: for a kernel / copy trace)
const fs = require('fs');
const { Cube, GenericDimension } = require('../olap-in-memory_amd/js');

const lines = [];
const say = (s) => {
  console.log(s);
  lines.push(s);
};
const now = () => process.hrtime.bigint();
const us = (t0) => Number(process.hrtime.bigint() - t0) / 1e3;
const median = (t) => t.slice().sort((a, b) => a - b)[Math.floor(t.length / 2)];
const fmt = (x) => (x === null ? 'skipped'.padStart(11) : (x >= 1e4 ? `${(x / 1e3).toFixed(1)} ms` : `${x.toFixed(1)} us`).padStart(11));

const dimsCache = {};
function dims(side) {
  if (!dimsCache[side]) {
    dimsCache[side] = ['r', 'c'].map((p) => new GenericDimension(p, 'item', Array.from({ length: side }, (_x, i) => `${p}${i}`)));
  }
  return dimsCache[side];
}

function fresh(side, rule) {
  const cube = new Cube(dims(side));
  cube.createStoredMeasure('mm', rule === 'first' ? { r: 'first', c: 'first' } : {}, 'float32', 0);
  return cube;
}

// `leaves` leaves spread evenly over a side x side cube, keys in ascending item order
function sparseObject(side, leaves) {
  const rows = 10 ** Math.floor(Math.log10(leaves) / 2);
  const cols = leaves / rows;
  const obj = {};
  for (let i = 0; i < rows; ++i) {
    const row = {};
    const r = Math.floor((i * side) / rows);
    for (let j = 0; j < cols; ++j) row[`c${Math.floor((j * side) / cols)}`] = 1 + ((i + j) % 7);
    obj[`r${r}`] = row;
  }
  return obj;
}

function measure(side, rule, obj, reps) {
  const walk = [];
  const setValues = [];
  const native = [];
  const batched = [];
  let lists = null;
  for (let k = 0; k < reps; ++k) {
    let cube = fresh(side, rule);
    const store = cube.storedMeasures.mm;
    store.setValues = (indexes, values) => {
      lists = [indexes, values];
    };
    let t0 = now();
    cube.hydrateFromSparseNestedObject('mm', obj);
    walk.push(us(t0));
    cube = fresh(side, rule);
    t0 = now();
    cube.storedMeasures.mm.setValues(lists[0], lists[1]);
    setValues.push(us(t0));
    cube = fresh(side, rule);
    const idx = Float64Array.from(lists[0]);
    const vals = Float64Array.from(lists[1]);
    const writable = cube.storedMeasures.mm._writable;
    t0 = now();
    writable.setValues(idx, vals, undefined);
    native.push(us(t0));
    cube = fresh(side, rule);
    t0 = now();
    cube.hydrateFromSparseNestedObject('mm', obj);
    batched.push(us(t0));
  }
  return { walk: median(walk), setValues: median(setValues), native: median(native), batched: median(batched), n: lists[0].length };
}

if (process.argv[2] === '--native') {
  const n = Number(process.argv[3] || 1e6);
  const cube = fresh(1000, 'sum');
  const idx = Float64Array.from({ length: n }, (_x, i) => i % 1e6);
  const vals = Float64Array.from({ length: n }, (_x, i) => 1 + (i % 7));
  for (let k = 0; k < 5; ++k) {
    const t0 = now();
    cube.storedMeasures.mm._writable.setValues(idx, vals, undefined);
    console.log(`setValues native, ${n} entries: ${fmt(us(t0))}`);
  }
  process.exit(0);
}

for (const side of [1000, 10000]) {
  say(`# ${side * side} cells (${side} x ${side}), Float32, default 0; median of the runs per column`);
  say(`${'measure'.padEnd(8)} ${'leaves'.padStart(8)} ${'walk'.padStart(11)} ${'setValues'.padStart(11)} ${'native'.padStart(11)} ${'batched'.padStart(11)} ${'per-cell'.padStart(11)} ${'per leaf'.padStart(11)} ${'speed-up'.padStart(9)}`);
  for (const rule of ['sum', 'first']) {
    for (const leaves of [1e3, 1e5, 1e6]) {
      const obj = sparseObject(side, leaves);
      const r = measure(side, rule, obj, leaves >= 1e6 ? 3 : 5);
      let perCell = null;
      if (r.n <= 1e5 || (side === 1000 && rule === 'sum')) {
        const cube = fresh(side, rule);
        const t0 = now();
        cube._hydrateFromSparseNestedObjectPerCell('mm', obj);
        perCell = us(t0);
      }
      const speedup = perCell === null ? '' : `${(perCell / r.batched).toFixed(0)}x`;
      say(`${rule.padEnd(8)} ${String(r.n).padStart(8)} ${fmt(r.walk)} ${fmt(r.setValues)} ${fmt(r.native)} ${fmt(r.batched)} ${fmt(perCell)} ${fmt(perCell === null ? null : perCell / r.n)} ${speedup.padStart(9)}`);
    }
  }
}
if (process.argv[2]) fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
