'use strict';
/*
 * Cube.quantile / Cube.median over several stored measures without a GPU: the measures held whole on one device —
 * tracked ones included — leave in ONE quantileMulti call with the lengths, the dimension's index, the group map of the
 * attribute and q; sharded measures and stores of another class are selected on the host (_quantileHost); the result
 * has drillUp's dimensions and carries rules and computed measures; the errors.  The addon is a stub behind
 * backend.load() and the device stores are stubs behind real HipStore objects; js/cube.js and js/store/hip.js run as
 * they are.
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
      throw new Error(`Unsupported aggregation method: ${name}`); // a quantile consults no rule
    },
    shardWorld: () => 0,
    quantileMulti: (natives, lens, axis, q, groups, nGroups, launchesOut) => {
      calls.many.push({ op: 'quantileMulti', natives: natives.map((n) => n.name), lens: Array.from(lens), axis, q, groups: groups && Array.from(groups), nGroups });
      launchesOut[0] = 1;
      const size = product(lens) / lens[axis] * nGroups;
      return natives.map((n) => stubNative(`quantileMulti(${n.name})`, size, calls));
    },
  };
  backend.load = () => addon;
  HipStore.lastBatchLaunches = null;
  HipStore.lastQuantilePath = null;
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

describe('the eligible measures leave in one quantileMulti call', () => {
  it('three measures, tracked ones included, by year', () => {
    const { cube, calls } = stubCube(['a', 'ordered', 'mean'], { ordered: { orderTracked: 1 } });
    withStubbedAddon(calls, () => {
      const result = cube.quantile('time', 'year', 0.9);
      assert.equal(calls.many.length, 1);
      assert.equal(calls.single.length, 0);
      assert.deepEqual(calls.many[0], { op: 'quantileMulti', natives: ['a', 'ordered', 'mean'], lens: [3, 6, 2], axis: 1, q: 0.9, groups: [0, 0, 0, 0, 1, 1], nGroups: 2 });
      assert.equal(HipStore.lastQuantilePath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      assert.equal(calls.created.length, 0);
      // the result has drillUp's dimensions and carries rules and computed measures
      const rolled = cube.dimensions[1].drillUp('year');
      assert.deepEqual(result.dimensions.map((d) => [d.id, d.rootAttribute, d.numItems]), [['d1', 'item', 3], ['time', 'year', 2], ['d2', 'item', 2]]);
      assert.deepEqual(result.dimensions[1].getItems(), rolled.getItems());
      assert.ok(result.dimensions[0] === cube.dimensions[0] && result.dimensions[2] === cube.dimensions[2]);
      assert.equal(result.storedMeasures.mean._nativeStore.name, 'quantileMulti(mean)');
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

  it("'all' is one group without a map; median is quantile(0.5)", () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      const result = cube.median('d1', 'all');
      assert.deepEqual(calls.many[0], { op: 'quantileMulti', natives: ['a', 'mean'], lens: [3, 6, 2], axis: 0, q: 0.5, groups: null, nGroups: 1 });
      assert.deepEqual(result.dimensions.map((d) => d.numItems), [1, 6, 2]);
      calls.many.length = 0;
      cube.quantile('d1', 'all', 0.5);
      assert.deepEqual(calls.many[0].q, 0.5);
      cube.quantile('time', 'year', 0);
      cube.quantile('time', 'year', 1);
      assert.deepEqual(calls.many.map((c) => c.q), [0.5, 0, 1]);
    });
  });

  it('a cube of one measure is a batch of one', () => {
    const { cube, calls } = stubCube(['a']);
    withStubbedAddon(calls, () => {
      cube.median('time', 'year');
      assert.deepEqual(calls.many.map((c) => c.natives), [['a']]);
      assert.equal(HipStore.lastQuantilePath, 'device');
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
      cube.dice('d1', 'item', ['c', 'a']).median('time', 'year');
      assert.deepEqual(calls.many.map((c) => c.op), ['diceMulti', 'quantileMulti']);
      assert.deepEqual(calls.many[1].natives, ['diceMulti(a)', 'diceMulti(mean)']);
      assert.deepEqual(calls.many[1].lens, [2, 6, 2]);
      assert.equal(HipStore.lastBatchLaunches, 2);
    });
  });
});

describe('what is selected on the host', () => {
  it('sharded measures take _quantileHost, the others the call', () => {
    const { cube, calls } = stubCube(['a', 'split', 'mean'], { split: { isSharded: true } });
    withStubbedAddon(calls, () => {
      const result = cube.quantile('time', 'year', 0.5);
      assert.deepEqual(calls.many.map((c) => [c.op, c.natives]), [['quantileMulti', ['a', 'mean']]]);
      assert.equal(HipStore.lastQuantilePath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
      // the selected cells are written into ONE new store of the result's size
      assert.equal(calls.created.length, 1);
      assert.equal(calls.created[0].size, 12);
      assert.deepEqual(result.storedMeasureIds, ['a', 'split', 'mean']);
      assert.equal(result.storedMeasures.split._nativeStore.name, 'new');
      // cells are 0 (unset), 1, 2, ...: cell (d1 0, year 0, d2 0) has members 2, 4, 6 (quarter 0 holds cell 0, unset)
      const values = Array.from(calls.created[0].values);
      assert.equal(values[0], 4);
      assert.equal(values[1], (1 + 3 + 5 + 7) / 4); // d2 1: members 1 3 5 7, h = 1.5
      assert.equal(values[2], (8 + 10) / 2); // year 1 of d1 0: quarters 4, 5
    });
  });

  it('an addon without the call: every measure on the host', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      delete backend.load().quantileMulti;
      const result = cube.quantile('time', 'year', 0.25);
      assert.equal(calls.many.length, 0);
      assert.equal(HipStore.lastQuantilePath, 'host');
      assert.equal(calls.created.length, 2);
      assert.deepEqual(result.dimensions.map((d) => d.numItems), [3, 2, 2]);
    });
  });

  it('stores of another class are selected on the host from data and the status map', () => {
    class Plain {
      constructor(size, type = 'float64', defaultValue = 0) {
        Object.assign(this, { size, _type: type, _defaultValue: defaultValue, _dataMap: new Map() });
      }

      get data() {
        return Array.from({ length: this.size }, (_, i) => (this._dataMap.has(i) ? this._dataMap.get(i) : this._defaultValue));
      }

      set data(values) {
        values.forEach((v, i) => {
          if (v !== this._defaultValue) this._dataMap.set(i, v);
        });
      }
    }
    const cube = new Cube([new GenericDimension('d0', 'item', ['a', 'b', 'c', 'd']), new GenericDimension('d1', 'item', ['x', 'y'])]);
    const m = new Plain(8);
    [0.7, 5, 0, 9, 0.1, 0, 0, 7].forEach((v, i) => {
      if (v !== 0) m._dataMap.set(i, v);
    });
    cube.storedMeasures.m = m;
    cube.storedMeasuresRules.m = {};
    const result = cube.quantile('d0', 'all', 0.3);
    assert.ok(result.storedMeasures.m instanceof Plain && result.storedMeasures.m !== m);
    assert.deepEqual(result.storedMeasures.m.data, [0.28, 5 + 0.6 * 2]); // (0.1, 0.7; 0.3) unfused: 0.28; members 5 7 9: h = 0.6
    assert.deepEqual(cube.median('d0', 'all').storedMeasures.m.data, [(0.1 + 0.6 * 0.5), 7]);
    assert.equal(HipStore.lastQuantilePath, 'host');
    assert.equal(m._dataMap.size, 5);
  });
});

describe('errors and the trivial case', () => {
  it('an unknown dimension, an unknown attribute and a q outside [0, 1] throw', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      assert.throws(() => cube.quantile('nowhere', 'all', 0.5), /quantile: no such dimension: nowhere/);
      assert.throws(() => cube.quantile('time', 'fortnight', 0.5), /quantile: no such attribute: fortnight/);
      assert.throws(() => cube.median('d1', 'year'), /quantile: no such attribute: year/);
      assert.throws(() => cube._quantileHost('time', 'fortnight', 0.5), /quantile: no such attribute: fortnight/);
      for (const q of [-0.1, 1.5, Number.NaN, '0.5', undefined, null]) {
        assert.throws(() => cube.quantile('time', 'year', q), /quantile: q must lie in \[0, 1\]/);
        assert.throws(() => cube._quantileHost('time', 'year', q), /quantile: q must lie in \[0, 1\]/);
      }
      assert.equal(calls.many.length + calls.single.length, 0);
    });
  });

  it('the root attribute needs no pass: a clone', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    withStubbedAddon(calls, () => {
      const same = cube.quantile('time', 'quarter', 0.9);
      assert.equal(calls.many.length, 0);
      assert.ok(same !== cube);
      assert.equal(same.storedMeasures.a._nativeStore.name, 'clone(a)');
    });
  });

  it('median stays refused as a rule', () => {
    const { cube, calls } = stubCube(['a', 'mean']);
    cube.storedMeasuresRules.a = { time: 'median' };
    withStubbedAddon(calls, () => {
      backend.load().cumulateMulti = () => assert.ok(false);
      assert.throws(() => cube.cumulate('time'), /Unsupported aggregation method: median/);
      assert.equal(cube.median('time', 'year').storedMeasures.a._size, 12); // ... and is not consulted by the call
    });
  });
});

run();
