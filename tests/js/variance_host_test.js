'use strict';
/*
 * Cube.variance / Cube.stddev over several stored measures without a GPU: the measures held whole on one device —
 * tracked ones included — leave in ONE varianceMulti call with the lengths, the dimension's index, kind, ddof and the
 * group map of the attribute; sharded measures and stores of another class are folded on the host (_varianceHost, which
 * is pinned against hand-worked literals here); the result has drillUp's dimensions and carries rules and computed
 * measures; the errors.  The addon is a stub behind backend.load() and the device stores are stubs behind real HipStore
 * objects; js/cube.js and js/store/hip.js run as they are.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, HipStore, backend } = require('../../olap-in-memory_amd/js');

const product = (lens) => Array.from(lens).reduce((n, l) => n * l, 1);

// a device store that only records what it is asked; its cells are 1, 2, 3, ... (cell 0 unset under the 0 default)
function stubNative(name, size, calls, { isSharded = false, orderTracked = 0 } = {}) {
  const cells = Float64Array.from({ length: size }, (_, i) => i);
  const self = {
    name,
    size,
    dtype: 2,
    isSharded,
    orderTracked,
    getDataF64: () => cells,
    getKeys: () => Array.from({ length: size - 1 }, (_, i) => i + 1),
    gather: () => (calls.single.push({ op: 'gather', name }), stubNative(`gather(${name})`, size, calls)),
    clone: () => stubNative(`clone(${name})`, size, calls, { isSharded, orderTracked }),
    trackOrder: () => {
      self.orderTracked = 1;
    },
  };
  return self;
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
      throw new Error(`Unsupported aggregation method: ${name}`); // a variance consults no rule
    },
    shardWorld: () => 0,
    varianceMulti: (natives, lens, axis, kind, ddof, groups, nGroups, launchesOut) => {
      calls.many.push({ op: 'varianceMulti', natives: natives.map((n) => n.name), lens: Array.from(lens), axis, kind, ddof, groups: groups && Array.from(groups), nGroups });
      launchesOut[0] = 1;
      const size = product(lens) / lens[axis] * nGroups;
      return natives.map((n) => stubNative(`varianceMulti(${n.name})`, size, calls));
    },
  };
  backend.load = () => addon;
  HipStore.lastBatchLaunches = null;
  HipStore.lastVariancePath = null;
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
    cube.storedMeasuresRules[id] = { time: id === 'ordered' ? 'last' : id === 'mean' ? 'average' : 'sum', d1: 'sum', d2: 'sum' };
  }
  cube.createComputedMeasure('twice', `2 * ${ids[0]}`);
  return { cube, calls };
}

// a store of another class: data and the status map are all _varianceHost reads
class Plain {
  constructor(size, type = 'float64', defaultValue = 0) {
    Object.assign(this, { size, _type: type, _defaultValue: defaultValue, _dataMap: new Map() });
  }

  get data() {
    return Array.from({ length: this.size }, (_, i) => (this._dataMap.has(i) ? this._dataMap.get(i) : this._defaultValue));
  }

  set data(values) {
    values.forEach((v, i) => {
      if (!Object.is(v, this._defaultValue) && !(v === 0 && this._defaultValue === 0)) this._dataMap.set(i, v);
    });
  }
}

function plainCube(dimensions, cells, defaultValue = 0) {
  const cube = new Cube(dimensions);
  const m = new Plain(cells.length, 'float64', defaultValue);
  cells.forEach((v, i) => {
    if (v !== null) m._dataMap.set(i, v);
  });
  cube.storedMeasures.m = m;
  cube.storedMeasuresRules.m = {};
  return cube;
}

describe('the eligible measures leave in one varianceMulti call', () => {
  it('three measures, tracked ones included, by year', () => {
    const { cube, calls } = stubCube(['a', 'ordered', 'mean'], { ordered: { orderTracked: 1 } });
    withStubbedAddon(calls, () => {
      const result = cube.variance('time', 'year', 1);
      assert.equal(calls.many.length, 1);
      assert.equal(calls.single.length, 0);
      assert.deepEqual(calls.many[0], { op: 'varianceMulti', natives: ['a', 'ordered', 'mean'], lens: [3, 6, 2], axis: 1, kind: 0, ddof: 1, groups: [0, 0, 0, 0, 1, 1], nGroups: 2 });
      assert.equal(HipStore.lastVariancePath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      assert.equal(calls.created.length, 0);
      // the result has drillUp's dimensions and carries rules and computed measures
      const rolled = cube.dimensions[1].drillUp('year');
      assert.deepEqual(result.dimensions.map((d) => [d.id, d.rootAttribute, d.numItems]), [['d1', 'item', 3], ['time', 'year', 2], ['d2', 'item', 2]]);
      assert.deepEqual(result.dimensions[1].getItems(), rolled.getItems());
      assert.ok(result.dimensions[0] === cube.dimensions[0] && result.dimensions[2] === cube.dimensions[2]);
      assert.equal(result.storedMeasures.mean._nativeStore.name, 'varianceMulti(mean)');
      assert.equal(result.storedMeasures.mean._size, 12);
      assert.deepEqual(result.storedMeasureIds, cube.storedMeasureIds);
      assert.ok(result.storedMeasuresRules.mean === cube.storedMeasuresRules.mean);
      assert.deepEqual(result.computedMeasureIds, ['twice']);
      // tracking is turned on afterwards where the rules ask for it, as _newStore does
      assert.equal(result.storedMeasures.ordered._nativeStore.orderTracked, 1);
      assert.equal(result.storedMeasures.a._nativeStore.orderTracked, 0);
      assert.equal(cube.storedMeasures.a._nativeStore.name, 'a'); // the source cube is untouched
      assert.equal(cube.dimensions[1].numItems, 6);
    });
  });

  it("'all' is one group without a map; stddev is kind 1; ddof defaults to 0", () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      const result = cube.stddev('d1', 'all');
      assert.deepEqual(calls.many[0], { op: 'varianceMulti', natives: ['a', 'mean'], lens: [3, 6, 2], axis: 0, kind: 1, ddof: 0, groups: null, nGroups: 1 });
      assert.deepEqual(result.dimensions.map((d) => d.numItems), [1, 6, 2]);
      calls.many.length = 0;
      cube.variance('time', 'year');
      cube.variance('time', 'year', 1);
      cube.stddev('time', 'year', 1);
      assert.deepEqual(calls.many.map((c) => [c.kind, c.ddof]), [[0, 0], [0, 1], [1, 1]]);
    });
  });

  it('the root attribute is not special: as many groups as items', () => {
    const { cube, calls } = stubCube(['a']);
    withStubbedAddon(calls, () => {
      const result = cube.variance('time', 'quarter');
      assert.deepEqual(calls.many.map((c) => [c.natives, c.groups, c.nGroups]), [[['a'], [0, 1, 2, 3, 4, 5], 6]]);
      assert.equal(result.storedMeasures.a._nativeStore.name, 'varianceMulti(a)');
      assert.deepEqual(result.dimensions.map((d) => d.numItems), [3, 6, 2]);
      assert.equal(HipStore.lastVariancePath, 'device');
    });
  });

  it('pending selections are diced first and go with the call', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      const addon = backend.load();
      addon.diceMulti = (natives, oldLen, midLen, sel, launchesOut) => {
        calls.many.push({ op: 'diceMulti', natives: natives.map((n) => n.name) });
        launchesOut[0] = 1;
        return natives.map((n) => stubNative(`diceMulti(${n.name})`, product(midLen), calls));
      };
      cube.dice('d1', 'item', ['c', 'a']).stddev('time', 'year');
      assert.deepEqual(calls.many.map((c) => c.op), ['diceMulti', 'varianceMulti']);
      assert.deepEqual(calls.many[1].natives, ['diceMulti(a)', 'diceMulti(mean)']);
      assert.deepEqual(calls.many[1].lens, [2, 6, 2]);
      assert.equal(HipStore.lastBatchLaunches, 2);
    });
  });
});

describe('what is folded on the host', () => {
  it('sharded measures take _varianceHost, the others the call', () => {
    const { cube, calls } = stubCube(['a', 'split', 'mean'], { split: { isSharded: true } });
    withStubbedAddon(calls, () => {
      const result = cube.variance('time', 'year');
      assert.deepEqual(calls.many.map((c) => [c.op, c.natives]), [['varianceMulti', ['a', 'mean']]]);
      assert.equal(HipStore.lastVariancePath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      // the folded cells are written into ONE new store of the result's size
      assert.equal(calls.created.length, 1);
      assert.equal(calls.created[0].size, 12);
      assert.deepEqual(result.storedMeasureIds, ['a', 'split', 'mean']);
      assert.equal(result.storedMeasures.split._nativeStore.name, 'new');
      // cells are 0 (unset), 1, 2, ...: cell (d1 0, year 0, d2 0) has members 2, 4, 6 (quarter 0 holds cell 0, unset)
      const values = Array.from(calls.created[0].values);
      assert.equal(values[0], 8 / 3);
      assert.equal(values[1], 5); // d2 1: members 1 3 5 7, mean 4, m2 20
      assert.equal(values[2], 1); // year 1 of d1 0: quarters 4, 5 hold 8 and 10
    });
  });

  it('an addon without the call: every measure on the host', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      delete backend.load().varianceMulti;
      const result = cube.stddev('time', 'year', 1);
      assert.equal(calls.many.length, 0);
      assert.equal(HipStore.lastVariancePath, 'host');
      assert.equal(calls.created.length, 2);
      assert.deepEqual(result.dimensions.map((d) => d.numItems), [3, 2, 2]);
      assert.equal(Array.from(calls.created[0].values)[1], Math.sqrt(20 / 3));
    });
  });
});

describe('_varianceHost is the definition', () => {
  const eight = [2, 4, 4, 4, 5, 5, 7, 9];
  const items = (n) => Array.from({ length: n }, (_, i) => `i${i}`);

  it('hand-worked literals: 4, 2 and 32 / 7', () => {
    const cube = plainCube([new GenericDimension('d0', 'item', items(8))], eight);
    assert.deepEqual(cube._varianceHost('d0', 'all', 0, 0).storedMeasures.m.data, [4]);
    assert.deepEqual(cube._varianceHost('d0', 'all', 0, 1).storedMeasures.m.data, [2]);
    assert.deepEqual(cube._varianceHost('d0', 'all', 1, 0).storedMeasures.m.data, [32 / 7]);
    assert.deepEqual(cube._varianceHost('d0', 'all', 1, 1).storedMeasures.m.data, [Math.sqrt(32 / 7)]);
    assert.deepEqual(cube.variance('d0', 'all').storedMeasures.m.data, [4]);
    assert.deepEqual(cube.stddev('d0', 'all', 1).storedMeasures.m.data, [Math.sqrt(32 / 7)]);
    assert.equal(HipStore.lastVariancePath, 'host');
    assert.ok(cube.variance('d0', 'all').storedMeasures.m instanceof Plain);
    assert.equal(cube.storedMeasures.m._dataMap.size, 8); // this cube is untouched
  });

  it('interleaved groups, unset cells, a group without members, along either dimension', () => {
    const d0 = new GenericDimension('d0', 'item', items(6));
    d0.addAttribute('item', 'parity', (item) => (Number(item.slice(1)) % 2 ? 'odd' : 'even'));
    // rows are items of d0, columns x and y; null: unset
    const cube = plainCube([d0, new GenericDimension('d1', 'item', ['x', 'y'])], [1, null, 10, 3, 3, null, 20, 3, 8, null, null, 3]);
    // even: x 1 3 8 (mean 4, m2 26), y none;  odd: x 10 20 (mean 15, m2 50), y 3 3 3
    assert.deepEqual(cube._varianceHost('d0', 'parity', 0, 0).storedMeasures.m.data, [26 / 3, 0, 25, 0]);
    assert.deepEqual(cube._varianceHost('d0', 'parity', 1, 0).storedMeasures.m.data, [13, 0, 50, 0]);
    assert.deepEqual(Array.from(cube._varianceHost('d0', 'parity', 1, 1).storedMeasures.m._dataMap.keys()), [0, 2]); // a variance of 0 is unset under the 0 default
    assert.deepEqual(cube._varianceHost('d1', 'all', 0, 0).storedMeasures.m.data, [0, 12.25, 0, 72.25, 0, 0]);
  });

  it('one member: 0 — unset under a 0 default, a set 0 under a NaN default — and unset with ddof 1; the root attribute', () => {
    const dims = () => [new GenericDimension('d0', 'item', items(3))];
    const zero = plainCube(dims(), [7, null, 5]);
    assert.equal(zero._varianceHost('d0', 'item', 0, 0).storedMeasures.m._dataMap.size, 0);
    assert.equal(zero._varianceHost('d0', 'item', 1, 0).storedMeasures.m._dataMap.size, 0);
    const nan = plainCube(dims(), [7, null, 5], Number.NaN);
    assert.deepEqual(Array.from(nan._varianceHost('d0', 'item', 0, 1).storedMeasures.m._dataMap.entries()), [[0, 0], [2, 0]]);
    assert.equal(nan._varianceHost('d0', 'item', 1, 0).storedMeasures.m._dataMap.size, 0);
    assert.deepEqual(Array.from(nan.variance('d0', 'item').storedMeasures.m._dataMap.keys()), [0, 2]); // no clone for the root attribute
    assert.deepEqual(nan.variance('d0', 'all', 1).storedMeasures.m.data, [2]);
  });

  it('a large common offset keeps its digits; ±Infinity and a set NaN give NaN', () => {
    const offset = plainCube([new GenericDimension('d0', 'item', items(8))], eight.map((_, k) => 1e9 + k));
    assert.deepEqual(offset._varianceHost('d0', 'all', 0, 0).storedMeasures.m.data, [5.25]);
    assert.deepEqual(offset._varianceHost('d0', 'all', 1, 0).storedMeasures.m.data, [6]);
    for (const cells of [[Infinity, 1, 2], [-Infinity, 1, 2], [Infinity, -Infinity, 2], [1, Number.NaN, 2]]) {
      const cube = plainCube([new GenericDimension('d0', 'item', items(3))], cells);
      for (const kind of [0, 1]) {
        const out = cube._varianceHost('d0', 'all', 0, kind).storedMeasures.m;
        assert.ok(out._dataMap.size === 1 && Number.isNaN(out._dataMap.get(0))); // a set NaN under the 0 default
      }
      const under = plainCube([new GenericDimension('d0', 'item', items(3))], cells.filter((v) => !Number.isNaN(v)).concat(cells.some(Number.isNaN) ? [null] : []), Number.NaN);
      if (!cells.some(Number.isNaN)) assert.equal(under._varianceHost('d0', 'all', 0, 0).storedMeasures.m._dataMap.size, 0); // NaN is the default: unset
    }
  });
});

describe('errors', () => {
  it('an unknown dimension, an unknown attribute and a ddof other than 0 or 1 throw', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      assert.throws(() => cube.variance('nowhere', 'all'), /variance: no such dimension: nowhere/);
      assert.throws(() => cube.stddev('nowhere', 'all'), /variance: no such dimension: nowhere/);
      assert.throws(() => cube.variance('time', 'fortnight'), /variance: no such attribute: fortnight/);
      assert.throws(() => cube.stddev('d1', 'year', 1), /variance: no such attribute: year/);
      assert.throws(() => cube._varianceHost('time', 'fortnight', 0, 0), /variance: no such attribute: fortnight/);
      for (const ddof of [-1, 2, 0.5, Number.NaN, '1', null, true]) {
        assert.throws(() => cube.variance('time', 'year', ddof), /variance: ddof must be 0 or 1/);
        assert.throws(() => cube.stddev('time', 'year', ddof), /variance: ddof must be 0 or 1/);
        assert.throws(() => cube._varianceHost('time', 'year', ddof, 0), /variance: ddof must be 0 or 1/);
      }
      assert.throws(() => cube._varianceHost('time', 'year', 0, 2), /variance: kind must be 0 or 1/);
      assert.equal(calls.many.length + calls.single.length, 0);
    });
  });

  it('no rule is consulted', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    cube.storedMeasuresRules.a = { time: 'median' };
    withStubbedAddon(calls, () => {
      assert.equal(cube.variance('time', 'year').storedMeasures.a._size, 12);
    });
  });
});

run();
