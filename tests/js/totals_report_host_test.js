'use strict';
/*
 * Cube.getNestedObjects(ids, true) without a GPU: which ids leave in ONE report (HipStore.totalsReport ->
 * addon.totalsReport, olap_totals_report), which keep the per-measure calls and which the chain of drillUps, and what the
 * addon is handed.  The addon is a stub behind backend.load(); the stores are HipStore objects without a device behind
 * them; js/cube.js and HipStore.totalsReport run as they are.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, HipStore, backend } = require('../../olap-in-memory_amd/js');
const { getParser, OP } = require('../../olap-in-memory_amd/js/formula');

const RULE_CODES = { sum: 0, average: 1, highest: 2, lowest: 3, first: 4, last: 5, product: 6 };

// a HipStore with no device behind it: `_whole` is a token the stub addon gets back, totals() the per-measure call
function stubStore(name, calls, ext, orderTracked = 0) {
  const store = Object.create(HipStore.prototype);
  Object.defineProperty(store, 'orderTracked', { value: orderTracked });
  Object.defineProperty(store, '_whole', { get: () => `native:${name}` });
  Object.defineProperty(store, 'totals', { value: () => (calls.perMeasure.push(name), new Float64Array(ext).fill(7)) });
  return store;
}

function stubCube(lengths = [3, 2]) {
  const dims = lengths.map((n, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  const ext = lengths.reduce((n, l) => n * (l + 1), 1);
  const calls = { report: [], perMeasure: [], chain: [] };
  for (let k = 0; k < 10; ++k) {
    cube.storedMeasures[`m${k}`] = stubStore(`m${k}`, calls, ext);
    cube.storedMeasuresRules[`m${k}`] = { d0: k % 2 ? 'average' : 'sum' }; // (d1 left to the default)
  }
  cube.storedMeasures.tracked = stubStore('tracked', calls, ext, 1);
  cube.storedMeasuresRules.tracked = { d0: 'last' };
  cube._getNestedObjectsChain = (ids) => {
    calls.chain.push(ids.slice());
    return Object.fromEntries(ids.map((id) => [id, `chain:${id}`]));
  };
  const formula = (id, text) => {
    cube.computedMeasures[id] = getParser().parse(text);
  };
  return { cube, calls, formula, ext };
}

// runs fn with a stub addon (with or without totalsReport) and a stub of the per-measure formula call
function withStubbedAddon(calls, { report = true } = {}, fn) {
  const realLoad = backend.load;
  const realFormula = HipStore.totalsFormula;
  const addon = {
    methodFromName: (name) => {
      if (name !== undefined && RULE_CODES[name] === undefined) throw new Error(`Unsupported aggregation method: ${name}`);
      return name === undefined ? 0 : RULE_CODES[name];
    },
  };
  if (report) {
    addon.totalsReport = (natives, lens, codes, outStored, nCode, code, nConsts, consts, nInputs, picks, launchesOut) => {
      calls.report.push({ natives, lens, codes, outStored, nCode, code, nConsts, consts, nInputs, picks });
      const ext = Array.from(lens).reduce((n, l) => n * (l + 1), 1);
      const values = new Float64Array(outStored.length * ext);
      for (let k = 0; k < outStored.length; ++k) values.fill(100 + k, k * ext, (k + 1) * ext); // slot k holds 100 + k
      launchesOut[0] = 5;
      return values;
    };
  }
  backend.load = () => addon;
  HipStore.totalsFormula = (program, inputs) => {
    calls.perMeasure.push(`formula over ${inputs.map((s) => s._whole.slice(7)).join(',')}`);
    return new Float64Array(calls.ext).fill(1);
  };
  HipStore.lastTotalsCalls = null;
  HipStore.lastTotalsLaunches = null;
  HipStore.lastTotalsPath = null;
  try {
    return fn();
  } finally {
    backend.load = realLoad;
    HipStore.totalsFormula = realFormula;
  }
}

// the INPUT operands of program k of a report call, as report input numbers
function operandsOf(call, k) {
  let at = 0;
  let pick = 0;
  for (let j = 0; j < k; ++j) {
    at += call.nCode[j];
    pick += call.nInputs[j];
  }
  const words = Array.from(call.code.slice(at, at + call.nCode[k]));
  const out = [];
  for (let pc = 0; pc < words.length; ++pc) {
    if (words[pc] === OP.INPUT) out.push(call.picks[pick + words[pc + 1]]);
    if (words[pc] === OP.INPUT || words[pc] === OP.CONST) ++pc;
  }
  return out;
}

describe('Cube.getNestedObjects(ids, true): one report for the eligible ids', () => {
  it('eligible, ineligible and duplicate ids: one report, the chain once, every distinct input once', () => {
    const { cube, calls, formula, ext } = stubCube();
    calls.ext = ext;
    formula('margin', 'm1 - m0');
    formula('pct', '(m1 - m0) / m1');
    formula('share', 'm0 / m0__total');
    formula('order', 'm0 + tracked');
    formula('third', 'm4 / 3');
    const ids = ['share', 'm0', 'margin', 'tracked', 'third', 'm0', 'order', 'pct', 'margin', 'share'];
    const out = withStubbedAddon(calls, {}, () => cube.getNestedObjects(ids, true));
    assert.deepEqual(Object.keys(out), ['share', 'm0', 'margin', 'tracked', 'third', 'order', 'pct']); // the caller's order
    assert.deepEqual(calls.chain, [['share', 'tracked', 'order']]);
    assert.equal(calls.perMeasure.length, 0);
    assert.equal(calls.report.length, 1);
    const call = calls.report[0];
    // outputs: m0, margin, third, pct — each id once, in the caller's order; inputs in order of first use
    assert.deepEqual(call.natives, ['native:m0', 'native:m1', 'native:m4']);
    assert.deepEqual(Array.from(call.outStored), [0, -1, -1, -1]);
    assert.deepEqual(Array.from(call.nInputs), [0, 2, 1, 2]);
    assert.deepEqual(Array.from(call.nCode).map((n) => n > 0), [false, true, true, true]);
    assert.equal(call.code.length, call.nCode.reduce((a, b) => a + b, 0));
    assert.equal(call.consts.length, call.nConsts.reduce((a, b) => a + b, 0));
    assert.equal(call.picks.length, 5);
    assert.deepEqual(operandsOf(call, 1), [1, 0]); // m1 - m0
    assert.deepEqual(operandsOf(call, 2), [2]); // m4 / 3
    assert.deepEqual(operandsOf(call, 3), [1, 0, 1]); // (m1 - m0) / m1
    assert.deepEqual(Array.from(call.consts), [3]);
    // each input's own rule per dimension: m0 sum, m1 average, m4 sum; d1 left to the default
    assert.deepEqual(Array.from(call.codes), [0, 0, 1, 0, 0, 0]);
    assert.deepEqual(Array.from(call.lens), [3, 2]);
    // slot k goes to the k-th eligible id; 'all' is the last key at every level
    assert.equal(out.m0.all.all, 100);
    assert.equal(out.margin.d0i0.d1i1, 101);
    assert.equal(out.third.all.d1i0, 102);
    assert.equal(out.pct.d0i2.all, 103);
    assert.deepEqual(Object.keys(out.margin), ['d0i0', 'd0i1', 'd0i2', 'all']);
    for (const id of ['share', 'tracked', 'order']) assert.equal(out[id], `chain:${id}`);
    assert.equal(HipStore.lastTotalsCalls, 1);
    assert.equal(HipStore.lastTotalsLaunches, 5);
    assert.equal(HipStore.lastTotalsPath, 'device');
  });

  it('stored ids only: one report, lastTotalsPath stays unset', () => {
    const { cube, calls, ext } = stubCube();
    calls.ext = ext;
    const out = withStubbedAddon(calls, {}, () => cube.getNestedObjects(['m3', 'm2', 'm3'], true));
    assert.equal(calls.report.length, 1);
    assert.deepEqual(calls.report[0].natives, ['native:m3', 'native:m2']);
    assert.deepEqual(Array.from(calls.report[0].outStored), [0, 1]);
    assert.deepEqual(Array.from(calls.report[0].codes), [1, 0, 0, 0]);
    assert.equal(calls.report[0].code.length + calls.report[0].picks.length, 0);
    assert.equal(out.m3.all.all, 100);
    assert.equal(out.m2.all.all, 101);
    assert.equal(HipStore.lastTotalsCalls, 1);
    assert.equal(HipStore.lastTotalsPath, null);
  });

  it('a single eligible id, even named twice or next to ineligible ones: no report', () => {
    const { cube, calls, formula, ext } = stubCube([2, 2, 2]);
    calls.ext = ext;
    formula('margin', 'm1 - m0');
    formula('share', 'm0 / m0__total');
    withStubbedAddon(calls, {}, () => {
      cube.getNestedObject('margin', true);
      assert.deepEqual(calls.perMeasure, ['formula over m1,m0']);
      assert.equal(HipStore.lastTotalsCalls, 1);
      cube.getNestedObjects(['m5', 'm5', 'share', 'tracked'], true);
      assert.deepEqual(calls.perMeasure, ['formula over m1,m0', 'm5']);
      assert.equal(HipStore.lastTotalsCalls, 1);
      cube.getNestedObjects(['share', 'tracked'], true);
      assert.equal(HipStore.lastTotalsCalls, 0);
    });
    assert.equal(calls.report.length, 0);
    assert.deepEqual(calls.chain, [['share', 'tracked'], ['share', 'tracked']]);
  });

  it('an addon without totalsReport: the per-measure calls', () => {
    const { cube, calls, formula, ext } = stubCube();
    calls.ext = ext;
    formula('margin', 'm1 - m0');
    const out = withStubbedAddon(calls, { report: false }, () => cube.getNestedObjects(['m0', 'margin', 'm1', 'm0'], true));
    assert.equal(calls.report.length, 0);
    assert.deepEqual(calls.perMeasure, ['m0', 'formula over m1,m0', 'm1']);
    assert.equal(out.m0.all.all, 7);
    assert.equal(out.margin.all.all, 1);
    assert.equal(HipStore.lastTotalsCalls, 3);
  });

  it('a report too large for one call: HipStore.totalsReport answers null and Cube asks measure by measure', () => {
    const { cube, calls, formula, ext } = stubCube();
    calls.ext = ext;
    formula('margin', 'm1 - m0');
    const huge = [{ numItems: 40000 }, { numItems: 40000 }]; // 1.6e9 extended cells: two outputs and one scratch input pass 4e9
    const outputs = [{ store: cube.storedMeasures.m0, rules: [] }, { program: cube._totalsFormula('margin').program, stores: [cube.storedMeasures.m1, cube.storedMeasures.m0], rulesPerInput: [[], []] }];
    withStubbedAddon(calls, {}, () => {
      assert.equal(HipStore.totalsReport(outputs, huge), null);
      assert.equal(calls.report.length, 0);
      assert.equal(HipStore.totalsReport(outputs.slice(0, 1), huge).length, 1); // one output alone fits
      assert.equal(calls.report.length, 1);
      // more than 32 outputs or 32 distinct stores do not fit one call either
      const small = cube.dimensions;
      const m0 = { store: cube.storedMeasures.m0, rules: [] };
      assert.equal(HipStore.totalsReport(Array.from({ length: 33 }, () => m0), small), null);
      assert.equal(HipStore.totalsReport(Array.from({ length: 33 }, (_, k) => ({ store: stubStore(`x${k}`, calls, ext), rules: [] })), small), null);
      assert.equal(calls.report.length, 1);
      const real = HipStore.totalsReport;
      HipStore.totalsReport = () => null;
      try {
        const out = cube.getNestedObjects(['m0', 'margin'], true);
        assert.equal(out.m0.all.all, 7);
        assert.equal(out.margin.all.all, 1);
      } finally {
        HipStore.totalsReport = real;
      }
      assert.deepEqual(calls.perMeasure, ['m0', 'formula over m1,m0']);
      assert.equal(HipStore.lastTotalsCalls, 2);
    });
  });

  it('an unknown rule throws before the device is asked', () => {
    const { cube, calls, ext } = stubCube();
    calls.ext = ext;
    cube.storedMeasuresRules.m2 = { d0: 'median' };
    assert.throws(() => withStubbedAddon(calls, {}, () => cube.getNestedObjects(['m1', 'm2'], true)), /^Error: Unsupported aggregation method: median$/);
    assert.equal(calls.report.length, 0);
  });

  it('without totals nothing changes', () => {
    const { cube, calls, ext } = stubCube();
    calls.ext = ext;
    cube.getData = () => new Float64Array(6).fill(2);
    const out = withStubbedAddon(calls, {}, () => cube.getNestedObjects(['m0', 'm1'], false));
    assert.equal(calls.report.length + calls.perMeasure.length + calls.chain.length, 0);
    assert.equal(out.m1.d0i2.d1i1, 2);
  });
});

run();
