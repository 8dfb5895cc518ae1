'use strict';
/*
 * Cube.rolling and Cube.shift over several stored measures without a GPU: the eligible measures leave in ONE
 * rollingMulti call with the rule of each, the window, the group map of the attribute and the dimension's index;
 * order-tracking and sharded measures go item by item (the dice -> drillUp chain of _rollingPerItem, which is not asked
 * for an empty window); the errors.  The addon is a stub behind backend.load() and the device stores are stubs behind
 * real HipStore objects; js/cube.js and js/store/hip.js run as they are.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, HipStore, backend } = require('../../olap-in-memory_amd/js');

const RULE_CODES = { sum: 0, average: 1, highest: 2, lowest: 3, first: 4, last: 5, product: 6 };
const product = (lens) => Array.from(lens).reduce((n, l) => n * l, 1);

// a device store that only records what it is asked
function stubNative(name, size, calls, { isSharded = false, orderTracked = 0 } = {}) {
  const derived = (op, n) => stubNative(`${op}(${name})`, n, calls, { isSharded, orderTracked });
  return {
    name,
    size,
    dtype: 2,
    isSharded,
    orderTracked,
    dice: (oldLen, midLen) => (calls.single.push({ op: 'dice', name }), derived('dice', product(midLen))),
    diceDrillUp: (oldLen, midLen, newLen) => (calls.single.push({ op: 'diceDrillUp', name }), derived('diceDrillUp', product(newLen))),
    drillUp: (oldLen, newLen) => (calls.single.push({ op: 'drillUp', name }), derived('drillUp', product(newLen))),
    getDataF64: () => new Float64Array(size),
    clone: () => derived('clone', size),
  };
}

function withStubbedAddon(calls, fn) {
  const realLoad = backend.load;
  class Store {
    constructor(size, dtype) {
      Object.assign(this, { size, dtype, isSharded: false, orderTracked: 0, name: 'new' });
      calls.created.push(this);
    }

    setData(values) {
      this.values = values;
    }

    trackOrder() {
      this.orderTracked = 1;
    }
  }
  const addon = {
    Store,
    methodFromName: (name) => {
      if (name !== undefined && RULE_CODES[name] === undefined) throw new Error(`Unsupported aggregation method: ${name}`);
      return name === undefined ? 0 : RULE_CODES[name];
    },
    shardWorld: () => 0,
    rollingMulti: (natives, codes, lens, axis, before, after, groups, nGroups, launchesOut) => {
      calls.many.push({ op: 'rollingMulti', natives: natives.map((n) => n.name), codes: Array.from(codes), lens: Array.from(lens), axis, before, after, groups: groups && Array.from(groups), nGroups });
      launchesOut[0] = 1;
      return natives.map((n) => stubNative(`rollingMulti(${n.name})`, n.size, calls));
    },
  };
  backend.load = () => addon;
  HipStore.lastBatchLaunches = null;
  HipStore.lastRollingPath = null;
  try {
    return fn();
  } finally {
    backend.load = realLoad;
  }
}

function stubCube(ids, options = {}) {
  const dims = [new GenericDimension('d1', 'item', ['a', 'b', 'c']), new TimeDimension('time', 'quarter', '2010-Q1', '2011-Q2'),
    new GenericDimension('d2', 'item', ['x', 'y'])];
  const cube = new Cube(dims);
  const calls = { many: [], single: [], created: [] };
  for (const id of ids) {
    cube.storedMeasures[id] = new HipStore(36, 'float32', 0, stubNative(id, 36, calls, options[id]));
    cube.storedMeasuresRules[id] = { time: id === 'mean' ? 'average' : id === 'peak' ? 'highest' : 'sum', d1: 'sum', d2: 'sum' };
  }
  return { cube, calls };
}

describe('the eligible measures leave in one rollingMulti call', () => {
  it('three measures, a rule each, one group, the window as given', () => {
    const { cube, calls } = stubCube(['a', 'mean', 'peak']);
    withStubbedAddon(calls, () => {
      const rolled = cube.rolling('time', 2);
      assert.equal(calls.many.length, 1);
      assert.equal(calls.single.length, 0);
      assert.deepEqual(calls.many[0], { op: 'rollingMulti', natives: ['a', 'mean', 'peak'], codes: [0, 1, 2], lens: [3, 6, 2], axis: 1, before: 2, after: 0, groups: null, nGroups: 1 });
      assert.equal(HipStore.lastRollingPath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      assert.equal(rolled.storedMeasures.mean._nativeStore.name, 'rollingMulti(mean)');
      assert.ok(rolled !== cube && rolled.dimensions.length === 3 && rolled.storedMeasures.a._size === 36);
      assert.deepEqual(rolled.storedMeasureIds, cube.storedMeasureIds);
      assert.ok(rolled.storedMeasuresRules.mean === cube.storedMeasuresRules.mean);
      assert.equal(cube.storedMeasures.a._nativeStore.name, 'a'); // the source cube is untouched
    });
  });

  it('the group map of the attribute goes with the call; a centred window', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      cube.rolling('time', 1, 1, 'year');
      assert.deepEqual([calls.many[0].before, calls.many[0].after, calls.many[0].groups, calls.many[0].nGroups], [1, 1, [0, 0, 0, 0, 1, 1], 2]);
      calls.many.length = 0;
      cube.rolling('d1', 0, 1);
      assert.deepEqual([calls.many[0].axis, calls.many[0].before, calls.many[0].after, calls.many[0].groups], [0, 0, 1, null]);
    });
  });

  it('shift passes (offset, -offset)', () => {
    const { cube, calls } = stubCube(['a']);
    withStubbedAddon(calls, () => {
      cube.shift('time', 1);
      cube.shift('time', -4, 'year');
      cube.shift('time', 0);
      assert.deepEqual(calls.many.map((c) => [c.natives, c.before, c.after, c.nGroups]), [[['a'], 1, -1, 1], [['a'], -4, 4, 2], [['a'], 0, 0, 1]]);
      assert.ok(Object.is(calls.many[2].after, 0));
      assert.equal(calls.single.length, 0);
      assert.equal(HipStore.lastRollingPath, 'device');
    });
  });

  it('the root attribute is a grouping like any other: every item its own group', () => {
    const { cube, calls } = stubCube(['a']);
    withStubbedAddon(calls, () => {
      cube.rolling('time', 1, 0, 'quarter');
      assert.deepEqual([calls.many[0].groups, calls.many[0].nGroups], [[0, 1, 2, 3, 4, 5], 6]);
    });
  });
});

describe('what goes item by item', () => {
  it('tracked and sharded measures take the dice -> drillUp chain, the others the call', () => {
    const { cube, calls } = stubCube(['a', 'ordered', 'split', 'mean'], { ordered: { orderTracked: 1 }, split: { isSharded: true } });
    withStubbedAddon(calls, () => {
      const rolled = cube.rolling('time', 1, 0, 'year');
      assert.deepEqual(calls.many.map((c) => [c.op, c.natives]), [['rollingMulti', ['a', 'mean']]]);
      assert.equal(HipStore.lastRollingPath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      // one chain per item of the dimension and measure: 6 items x 2 measures reach a drillUp of some form
      const rolls = calls.single.filter((c) => c.op === 'drillUp' || c.op === 'diceDrillUp');
      assert.equal(rolls.length, 12);
      assert.ok(calls.single.every((c) => /ordered|split/.test(c.name)));
      assert.equal(calls.created.length, 2);
      assert.ok(calls.created.every((s) => s.size === 36 && s.values.length === 36));
      assert.deepEqual(rolled.storedMeasureIds, ['a', 'ordered', 'split', 'mean']);
      assert.equal(rolled.storedMeasures.ordered._nativeStore.name, 'new');
    });
  });

  it('the chain is not asked for an empty window', () => {
    const { cube, calls } = stubCube(['ordered'], { ordered: { orderTracked: 1 } });
    withStubbedAddon(calls, () => {
      cube.shift('time', 1, 'year'); // 2010-Q1 and 2011-Q1 have no quarter before them in their year
      assert.equal(calls.many.length, 0);
      assert.equal(HipStore.lastRollingPath, 'per-item');
      assert.equal(calls.single.filter((c) => c.op === 'drillUp' || c.op === 'diceDrillUp').length, 4);
      assert.equal(calls.created.length, 1);
    });
  });

  it('an addon without the call: per-item', () => {
    const { cube, calls } = stubCube(['a']);
    withStubbedAddon(calls, () => {
      delete backend.load().rollingMulti;
      cube.rolling('time', 1);
      assert.equal(calls.many.length, 0);
      assert.equal(HipStore.lastRollingPath, 'per-item');
      assert.equal(calls.created.length, 1);
    });
  });
});

describe('errors', () => {
  it('an unknown dimension, an unknown attribute, a window that is no window', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      assert.throws(() => cube.rolling('nowhere', 1), /rolling: no such dimension: nowhere/);
      assert.throws(() => cube.rolling('time', 1, 0, 'fortnight'), /rolling: no such attribute: fortnight in dimension: time/);
      assert.throws(() => cube.shift('d1', 1, 'year'), /rolling: no such attribute: year/);
      assert.throws(() => cube._rollingPerItem('time', 1, 0, 'fortnight'), /rolling: no such attribute: fortnight/);
      assert.throws(() => cube.rolling('time', 1.5), /rolling: before and after must be integers/);
      assert.throws(() => cube.rolling('time'), /rolling: before and after must be integers/);
      assert.throws(() => cube.rolling('time', 1, '0'), /rolling: before and after must be integers/);
      assert.throws(() => cube.rolling('time', 1, -2), /rolling: empty window/);
      assert.throws(() => cube._rollingPerItem('time', -1, 0), /rolling: empty window/);
      assert.equal(calls.many.length + calls.single.length, 0);
    });
  });

  it('an unsupported rule is refused by name', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    cube.storedMeasuresRules.a = { time: 'median' };
    withStubbedAddon(calls, () => {
      assert.throws(() => cube.rolling('time', 1), /Unsupported aggregation method: median/);
    });
  });
});

run();
