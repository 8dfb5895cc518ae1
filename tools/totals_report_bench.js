'use strict';
// Developer tool: cube.getNestedObjects(ids, true) over 2, 4 and 8 ids — half stored, half computed over the same stored
// measures — as ONE report (HipStore.totalsReport, olap_totals_report) against the per-measure calls of the same build
// (store.totals / HipStore.totalsFormula, one device call per id), in the same process, in alternating rounds (the two
// paths also take turns at going first); medians.
// `objects` is the whole getNestedObjects call, host formatting included; `calls` is the device calls alone.
// Usage: node tools/totals_report_bench.js [out.txt] [--aa]   (--aa: both sides run the per-measure path — the spread of the ratios)
const fs = require('fs');
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
const lengthsOf = (dimensions) => Uint32Array.from(dimensions, (d) => d.numItems);

// the reference's fixture (antennas / routers over location x period, uint32), with two more stored measures for the 8-id row
function fixture() {
  const period = new GenericDimension('period', 'season', ['summer', 'winter']);
  const location = new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']);
  const cube = new Cube([location, period]);
  const data = { antennas: [[1, 2], [4, 8], [16, 32]], routers: [[3, 2], [4, 9], [16, 32]], switches: [[2, 2], [3, 5], [9, 20]], cables: [[7, 1], [6, 6], [40, 64]] };
  for (const id of Object.keys(data)) {
    cube.createStoredMeasure(id, { period: 'sum', location: 'sum' }, 'uint32');
    cube.setNestedArray(id, data[id]);
  }
  cube.createComputedMeasure('router_by_antennas', 'routers / antennas');
  cube.createComputedMeasure('margin', 'routers - antennas');
  cube.createComputedMeasure('net', 'cables - switches');
  cube.createComputedMeasure('per_switch', 'cables / switches');
  return {
    label: 'fixture',
    cube,
    ids: { 2: ['routers', 'margin'], 4: ['routers', 'antennas', 'router_by_antennas', 'margin'], 8: ['routers', 'antennas', 'switches', 'cables', 'router_by_antennas', 'margin', 'net', 'per_switch'] },
  };
}

// a synthetic cube of four Float32 measures
function synthetic(lens) {
  const dims = lens.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  const n = cube.storeSize;
  ['revenue', 'cost', 'units', 'returns'].forEach((id, k) => {
    cube.createStoredMeasure(id, {}, 'float32', 0);
    cube.setData(id, Float32Array.from({ length: n }, (_, i) => ((i * (k + 3)) % 17) * 0.25));
  });
  const computed = { margin: 'revenue - cost', margin_pct: '(revenue - cost) / revenue', net: 'units - returns', price: 'revenue / units' };
  for (const id of Object.keys(computed)) cube.createComputedMeasure(id, computed[id]);
  return {
    label: `[${lens.join(',')}]`,
    cube,
    ids: { 2: ['revenue', 'margin'], 4: ['revenue', 'cost', 'margin', 'margin_pct'], 8: ['revenue', 'cost', 'units', 'returns', 'margin', 'margin_pct', 'net', 'price'] },
  };
}

const AA = process.argv.includes('--aa');
const canReport = AA ? () => false : HipStore.canReport;
if (AA) HipStore.canReport = canReport;
const perMeasure = (fn) => {
  HipStore.canReport = () => false;
  try {
    return fn();
  } finally {
    HipStore.canReport = canReport;
  }
};

if (AA) say('# A/A: both sides are the per-measure path');
say(`${'cube'.padStart(12)} ${'E cells'.padStart(8)} ${'ids'.padStart(3)} | ${'objects: per measure'.padStart(20)} ${'report'.padStart(11)} ${'ratio'.padStart(6)} | ${'calls: per measure'.padStart(18)} ${'report'.padStart(11)} ${'ratio'.padStart(6)} | launches per measure / report`);
for (const { label, cube, ids: idsOf } of [fixture(), synthetic([10, 10, 10]), synthetic([40, 40, 40])]) {
  const lens = Array.from(lengthsOf(cube.dimensions));
  const ext = lens.reduce((p, l) => p * (l + 1), 1);
  const rulesOf = (id) => cube.dimensions.map((d) => (cube.storedMeasuresRules[id] || {})[d.id]);
  const rounds = ext >= 1e4 ? 30 : 100;
  for (const count of [2, 4, 8]) {
    const ids = idsOf[count];
    const outputs = ids.map((id) => {
      if (cube.storedMeasures[id] !== undefined) return { store: cube.storedMeasures[id], rules: rulesOf(id) };
      const f = cube._totalsFormula(id);
      return { program: f.program, stores: f.stores, rulesPerInput: f.ids.map(rulesOf) };
    });
    let formulaLaunches = 0;
    const callsPerMeasure = () => {
      formulaLaunches = 0;
      for (const out of outputs) {
        if (out.program === undefined) {
          out.store.totals(cube.dimensions, out.rules);
        } else {
          HipStore.totalsFormula(out.program, out.stores, cube.dimensions, out.rulesPerInput);
          formulaLaunches += HipStore.lastTotalsLaunches;
        }
      }
    };
    const t = { objectsPer: [], objectsReport: [], callsPer: [], callsReport: [] };
    let launchesReport = 0;
    for (let r = -2; r < rounds; ++r) { // (two rounds warm both sides up)
      // the two paths take turns at going first: whatever the first leaves behind (garbage, warm caches) is shared out
      let a, b, c, d;
      const objectsPer = () => { a = clock(() => perMeasure(() => cube.getNestedObjects(ids, true))); };
      const objectsReport = () => {
        b = clock(() => cube.getNestedObjects(ids, true));
        if (!AA && HipStore.lastTotalsCalls !== 1) throw new Error('the report path did not run');
      };
      const callsPer = () => { c = clock(callsPerMeasure); };
      const callsReport = () => {
        d = clock(AA ? callsPerMeasure : () => HipStore.totalsReport(outputs, cube.dimensions));
        launchesReport = AA ? 0 : HipStore.lastTotalsLaunches;
      };
      for (const run of (r & 1 ? [objectsReport, objectsPer, callsReport, callsPer] : [objectsPer, objectsReport, callsPer, callsReport])) run();
      if (r >= 0) {
        t.objectsPer.push(a);
        t.objectsReport.push(b);
        t.callsPer.push(c);
        t.callsReport.push(d);
      }
    }
    // launches of the per-measure path: what each of its calls reports (olap_store_totals through the addon, outside the clock)
    const codes = Int32Array.from(lens, () => 0);
    const one = new Int32Array(1);
    let launchesPerMeasure = formulaLaunches;
    for (const out of outputs) {
      if (out.program !== undefined) continue;
      out.store._whole.totals(lengthsOf(cube.dimensions), codes, one);
      launchesPerMeasure += one[0];
    }
    const m = Object.fromEntries(Object.keys(t).map((k) => [k, median(t[k])]));
    say(`${label.padStart(12)} ${String(ext).padStart(8)} ${String(count).padStart(3)} | ${fmt(m.objectsPer).padStart(20)} ${fmt(m.objectsReport)} ${(m.objectsReport / m.objectsPer).toFixed(2).padStart(6)} | ${fmt(m.callsPer).padStart(18)} ${fmt(m.callsReport)} ${(m.callsReport / m.callsPer).toFixed(2).padStart(6)} | ${AA ? '-' : `${launchesPerMeasure} / ${launchesReport}`}`);
  }
}
if (process.argv[2] && process.argv[2] !== '--aa') fs.writeFileSync(process.argv[2], lines.join('\n') + '\n');
