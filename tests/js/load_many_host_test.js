'use strict';
/*
 * Cube.hydrateFromCube / reorderDimensions over several stored measures without a GPU: the measures two cubes share leave
 * in ONE loadMulti call with tables built once (HipStore.loadMany), a reorder in one reorderMulti (HipStore.reorderMany),
 * tracked and sharded measures keep the single-store calls, and a load between cell types never brings the source's
 * cells to the host.  The addon is a stub behind backend.load() and the device stores are stubs behind real HipStore
 * objects; js/cube.js and js/store/hip.js run as they are.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, HipStore, backend } = require('../../olap-in-memory_amd/js');

const DTYPE = { int32: 0, uint32: 1, float32: 2, float64: 3 };
const product = (lens) => Array.from(lens).reduce((n, l) => n * l, 1);

// a device store that only records what it is asked
function stubNative(name, size, calls, { dtype = 2, isSharded = false, orderTracked = 0 } = {}) {
  return {
    name,
    size,
    dtype,
    isSharded,
    orderTracked,
    load: (other, myLen, hisLen, maps) => { calls.single.push({ op: 'load', name, other: other.name, maps }); },
    reorder: (oldLen) => (calls.single.push({ op: 'reorder', name }), stubNative(`reorder(${name})`, product(oldLen), calls, { dtype, isSharded, orderTracked })),
    gather: () => (calls.single.push({ op: 'gather', name }), stubNative(`gather(${name})`, size, calls, { dtype, orderTracked })),
    getDataF64: () => (calls.single.push({ op: 'getDataF64', name }), new Float64Array(size)),
    setData: () => { calls.single.push({ op: 'setData', name }); },
    clone: () => stubNative(`clone(${name})`, size, calls, { dtype, isSharded, orderTracked }),
  };
}

function withStubbedAddon(calls, fn) {
  const realLoad = backend.load;
  const addon = {
    shardWorld: () => 0,
    Store: function Store(size, dtype) { return stubNative('retyped', size, calls, { dtype }); },
    loadMulti: (targets, sources, myLen, hisLen, maps, launchesOut) => {
      calls.many.push({ op: 'loadMulti', targets: targets.map((n) => n.name), sources: sources.map((n) => n.name), myLen, hisLen, maps });
      launchesOut[0] = 1;
    },
    reorderMulti: (natives, oldLen, perm, launchesOut) => {
      calls.many.push({ op: 'reorderMulti', natives: natives.map((n) => n.name), oldLen, perm });
      launchesOut[0] = 1;
      return natives.map((n) => stubNative(`reorderMulti(${n.name})`, product(oldLen), calls, { dtype: n.dtype }));
    },
  };
  backend.load = () => addon;
  HipStore.lastBatchLaunches = null;
  HipStore.lastLoadPath = null;
  try {
    return fn();
  } finally {
    backend.load = realLoad;
  }
}

// `types[id]`: [declared type, dtype of the cells]; `options[id]`: sharded / tracked
function stubCube(prefix, items1, items2, types, calls, options = {}) {
  const dims = [new GenericDimension('d1', 'item', items1), new GenericDimension('d2', 'item', items2)];
  const cube = new Cube(dims);
  const size = items1.length * items2.length;
  for (const id of Object.keys(types)) {
    const [type, cells] = types[id];
    cube.storedMeasures[id] = new HipStore(size, type, 0, stubNative(`${prefix}.${id}`, size, calls, Object.assign({ dtype: DTYPE[cells] }, options[id])));
    cube.storedMeasuresRules[id] = { d1: 'sum', d2: 'sum' };
  }
  return cube;
}

const MINE = { a: ['float32', 'float32'], b: ['float64', 'float64'], n: ['int32', 'float64'], k: ['int32', 'int32'] };
const HIS = { a: ['float64', 'float64'], b: ['float32', 'float32'], n: ['int32', 'int32'], k: ['float32', 'float32'], extra: ['float32', 'float32'] };

describe('the measures of a cube leave in one many-call', () => {
  it('hydrateFromCube: one loadMulti for four measures of other cell types, the tables built once', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y', 'z', 'w'], MINE, calls);
    const his = stubCube('his', ['b', 'c', 'q'], ['y', 'x'], HIS, calls);
    let tables = 0;
    for (const dim of mine.dimensions) {
      const real = dim.getItemsToIdx;
      dim.getItemsToIdx = function counted() {
        ++tables;
        return real.call(this);
      };
    }
    withStubbedAddon(calls, () => {
      mine.hydrateFromCube(his);
      assert.deepEqual(calls.many.map((c) => c.op), ['loadMulti']);
      assert.equal(calls.single.length, 0);
      const c = calls.many[0];
      assert.deepEqual(c.targets, ['mine.a', 'mine.b', 'mine.n', 'mine.k']);
      assert.deepEqual(c.sources, ['his.a', 'his.b', 'his.n', 'his.k']); // `extra` has no counterpart
      assert.deepEqual([Array.from(c.myLen), Array.from(c.hisLen)], [[3, 4], [3, 2]]);
      assert.deepEqual(c.maps.map((m) => Array.from(m)), [[1, 2, -1], [1, 0]]);
      assert.equal(tables, 2); // once per dimension, not once per measure
      assert.equal(HipStore.lastLoadPath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
    });
  });

  it('reorderDimensions: one reorderMulti', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y', 'z', 'w'], MINE, calls);
    withStubbedAddon(calls, () => {
      const swapped = mine.reorderDimensions(['d2', 'd1']);
      assert.deepEqual(calls.many.map((c) => c.op), ['reorderMulti']);
      assert.equal(calls.single.length, 0);
      assert.deepEqual(calls.many[0].natives, ['mine.a', 'mine.b', 'mine.n', 'mine.k']);
      assert.deepEqual([Array.from(calls.many[0].oldLen), Array.from(calls.many[0].perm)], [[3, 4], [1, 0]]);
      assert.equal(swapped.storedMeasures.n._nativeStore.name, 'reorderMulti(mine.n)');
      assert.equal(swapped.storedMeasures.n._type, 'int32');
      assert.deepEqual(swapped.dimensionIds, ['d2', 'd1']);
      assert.equal(HipStore.lastReorderLaunches, 1);
      assert.equal(HipStore.lastBatchLaunches, 0); // no pending selection had to be diced first
    });
  });
});

describe('what goes one by one', () => {
  it('tracked and sharded targets take load, sharded sources are gathered; tracked and sharded measures take reorder', () => {
    const calls = { many: [], single: [] };
    const options = { b: { orderTracked: 1 }, n: { isSharded: true } };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y', 'z', 'w'], { a: MINE.a, b: MINE.b, n: MINE.n, k: MINE.k }, calls, options);
    const his = stubCube('his', ['b', 'c', 'q'], ['y', 'x'], { a: MINE.a, b: MINE.b, n: MINE.n, k: MINE.k }, calls, { k: { isSharded: true } });
    withStubbedAddon(calls, () => {
      mine.hydrateFromCube(his);
      assert.deepEqual(calls.many.map((c) => [c.op, c.targets, c.sources]), [['loadMulti', ['mine.a', 'mine.k'], ['his.a', 'gather(his.k)']]]);
      assert.deepEqual(calls.single.filter((c) => c.op === 'load').map((c) => `${c.name} <- ${c.other}`), ['mine.b <- his.b', 'gather(mine.n) <- his.n']);
      assert.ok(calls.single.every((c) => c.op === 'load' || c.op === 'gather'));
      // the one-by-one loads got the tables of the many-call, not tables of their own
      assert.ok(calls.single.filter((c) => c.op === 'load').every((c) => c.maps === calls.many[0].maps));
      assert.equal(HipStore.lastLoadPath, 'device');
      calls.many.length = 0;
      calls.single.length = 0;
      // (the sharded target was gathered for its load and stays on one device: a cube as it was before is reordered)
      const fresh = stubCube('mine', ['a', 'b', 'c'], ['x', 'y', 'z', 'w'], { a: MINE.a, b: MINE.b, n: MINE.n, k: MINE.k }, calls, options);
      fresh.reorderDimensions(['d2', 'd1']);
      assert.deepEqual(calls.many.map((c) => [c.op, c.natives]), [['reorderMulti', ['mine.a', 'mine.k']]]);
      assert.deepEqual(calls.single.map((c) => `${c.op} ${c.name}`), ['reorder mine.b', 'reorder mine.n']);
    });
  });

  it('a cube of one measure makes no reorderMulti; stores of another class keep the per-measure calls', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b'], ['x', 'y'], { a: MINE.a }, calls);
    withStubbedAddon(calls, () => {
      mine.reorderDimensions(['d2', 'd1']);
      assert.equal(calls.many.length, 0);
      assert.deepEqual(calls.single.map((c) => c.op), ['reorder']);
    });
    const seen = [];
    const plain = (id) => ({ load: (other) => seen.push(`load ${id} <- ${other.id}`), reorder: () => (seen.push(`reorder ${id}`), plain(id)), id });
    const cube = new Cube([new GenericDimension('d1', 'item', ['a', 'b']), new GenericDimension('d2', 'item', ['x'])]);
    const other = new Cube([new GenericDimension('d1', 'item', ['a', 'b']), new GenericDimension('d2', 'item', ['x'])]);
    for (const id of ['m', 'n']) {
      cube.storedMeasures[id] = plain(id);
      cube.storedMeasuresRules[id] = {};
      other.storedMeasures[id] = plain(`other ${id}`);
      other.storedMeasuresRules[id] = {};
    }
    cube.hydrateFromCube(other);
    cube.reorderDimensions(['d2', 'd1']);
    assert.deepEqual(seen, ['load m <- other m', 'load n <- other n', 'reorder m', 'reorder n']);
  });
});

describe('load between cell types', () => {
  it('an untracked target: one loadMulti, the source\'s cells never come to the host', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y'], { a: MINE.a }, calls);
    const his = stubCube('his', ['a', 'b', 'c'], ['x', 'y'], { a: HIS.a }, calls);
    withStubbedAddon(calls, () => {
      mine.storedMeasures.a.load(his.storedMeasures.a, mine.dimensions, his.dimensions);
      assert.deepEqual(calls.many.map((c) => [c.op, c.targets, c.sources]), [['loadMulti', ['mine.a'], ['his.a']]]);
      assert.equal(calls.single.length, 0); // no getDataF64, no setData, no single-store load
      assert.equal(HipStore.lastLoadPath, 'device');
      assert.equal(HipStore.lastBatchLaunches, 1);
    });
  });

  it('a tracked target keeps the host path, and says so', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y'], { a: MINE.a }, calls, { a: { orderTracked: 1 } });
    const his = stubCube('his', ['a', 'b', 'c'], ['x', 'y'], { a: HIS.a }, calls);
    withStubbedAddon(calls, () => {
      mine.storedMeasures.a.load(his.storedMeasures.a, mine.dimensions, his.dimensions);
      assert.equal(calls.many.length, 0);
      assert.deepEqual(calls.single.map((c) => `${c.op} ${c.name}`), ['getDataF64 his.a', 'setData retyped', 'load mine.a']);
      assert.equal(calls.single[2].other, 'retyped');
      assert.equal(HipStore.lastLoadPath, 'host');
    });
  });

  it('a same-type load keeps the single-store call', () => {
    const calls = { many: [], single: [] };
    const mine = stubCube('mine', ['a', 'b', 'c'], ['x', 'y'], { a: MINE.a }, calls);
    const his = stubCube('his', ['a', 'b', 'c'], ['x', 'y'], { a: MINE.a }, calls);
    withStubbedAddon(calls, () => {
      mine.storedMeasures.a.load(his.storedMeasures.a, mine.dimensions, his.dimensions);
      assert.equal(calls.many.length, 0);
      assert.deepEqual(calls.single.map((c) => `${c.op} ${c.name}`), ['load mine.a']);
      assert.equal(HipStore.lastLoadPath, 'device');
    });
  });
});

run();
