'use strict';
/*
 * Cube.compose without a GPU: each source cube is reshaped once and its eligible stored measures leave in ONE composeMulti
 * call with the right fills (HipStore.composeMany); tracked and sharded measures keep create + fill + load and are loaded
 * once per source through loadMany; an addon without the call keeps the old calls; the composed cube carries both cubes'
 * computed measures.  The addon is a stub behind backend.load() and the device stores are stubs behind real HipStore
 * objects; js/cube.js and js/store/hip.js run as they are.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, HipStore, backend } = require('../../olap-in-memory_amd/js');

const DTYPE = { int32: 0, uint32: 1, float32: 2, float64: 3 };

// a device store that only records what it is asked
function stubNative(name, size, calls, { dtype = 2, isSharded = false, orderTracked = 0 } = {}) {
  const native = {
    name,
    size,
    dtype,
    isSharded,
    orderTracked,
    fill: (value) => { calls.single.push(`fill ${name} ${value}`); },
    trackOrder: (on) => {
      native.orderTracked = on ? 1 : 0;
      calls.single.push(`trackOrder ${name}`);
    },
    load: (other) => { calls.single.push(`load ${name} <- ${other.name}`); },
    gather: () => (calls.single.push(`gather ${name}`), stubNative(`gather(${name})`, size, calls, { dtype, orderTracked })),
    clone: () => stubNative(`clone(${name})`, size, calls, { dtype, isSharded, orderTracked }),
  };
  return native;
}

function withStubbedAddon(calls, fn, { world = 0, composeMulti = true } = {}) {
  const realLoad = backend.load;
  const realLoadMany = HipStore.loadMany;
  let created = 0;
  const addon = {
    shardWorld: () => world,
    Store: function Store(size, dtype) { return stubNative(`new${created++}`, size, calls, { dtype }); },
    ShardedStore: function ShardedStore(lengths, dtype) {
      return stubNative(`sharded${created++}`, Array.from(lengths).reduce((n, l) => n * l, 1), calls, { dtype, isSharded: true });
    },
    loadMulti: (targets, sources, myLen, hisLen, maps, launchesOut) => {
      calls.many.push({ op: 'loadMulti', targets: targets.map((n) => n.name), sources: sources.map((n) => n.name) });
      launchesOut[0] = 1;
    },
  };
  if (composeMulti) {
    addon.composeMulti = (sources, myLen, hisLen, maps, fills, hasFill, launchesOut) => {
      calls.many.push({ op: 'composeMulti', sources: sources.map((n) => n.name), myLen: Array.from(myLen), hisLen: Array.from(hisLen),
                        maps: maps.map((m) => Array.from(m)), fills: Array.from(fills), hasFill: Array.from(hasFill) });
      launchesOut[0] = 1;
      return sources.map((n) => stubNative(`composeMulti(${n.name})`, Array.from(myLen).reduce((k, l) => k * l, 1), calls, { dtype: n.dtype }));
    };
  }
  backend.load = () => addon;
  HipStore.loadMany = function counted(...args) {
    calls.loadMany += 1;
    return realLoadMany.apply(HipStore, args);
  };
  HipStore.lastBatchLaunches = null;
  HipStore.lastComposeCalls = -1;
  try {
    return fn();
  } finally {
    backend.load = realLoad;
    HipStore.loadMany = realLoadMany;
  }
}

// `types[id]`: [declared type, dtype of the cells]; `options[id]`: sharded / tracked; `rules[id]`: the measure's rules
function stubCube(prefix, items1, items2, types, calls, options = {}, rules = {}) {
  const dims = [new GenericDimension('d1', 'item', items1), new GenericDimension('d2', 'item', items2)];
  const cube = new Cube(dims);
  const size = items1.length * items2.length;
  for (const id of Object.keys(types)) {
    const [type, cells] = types[id];
    cube.storedMeasures[id] = new HipStore(size, type, 0, stubNative(`${prefix}.${id}`, size, calls, Object.assign({ dtype: DTYPE[cells] }, options[id])));
    cube.storedMeasuresRules[id] = rules[id] || { d1: 'sum', d2: 'sum' };
  }
  cube.reshapes = 0;
  const reshape = cube.reshape;
  cube.reshape = function counted(...args) {
    cube.reshapes += 1;
    return reshape.apply(this, args);
  };
  return cube;
}

const newCalls = () => ({ many: [], single: [], loadMany: 0 });
const F32 = ['float32', 'float32'];
const F64 = ['float64', 'float64'];
const I32 = ['int32', 'float64']; // integer measures live in Float64 cells
const twoCubes = (calls, optionsA = {}, rulesA = {}) => [
  stubCube('A', ['a', 'b', 'c'], ['x', 'y', 'z', 'w'], { aa: F32, bb: F64, nn: I32 }, calls, optionsA, rulesA),
  stubCube('B', ['b', 'c', 'q'], ['y', 'x'], { hh: F32 }, calls),
];
// his item -> my item, as load takes it
const mapsOnto = (cube, source) => source.dimensions.map((dim, i) => dim.getItems().map((item) => cube.dimensions[i].getItems().indexOf(item)));

describe('compose: one device call per source cube', () => {
  it('all eligible measures of a source in one composeMulti, the right fills, one reshape each', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    withStubbedAddon(calls, () => {
      const cube = A.compose(B, false, { aa: 7, nn: 2.5, hh: 0 });
      assert.deepEqual(calls.many.map((c) => [c.op, c.sources]), [['composeMulti', ['A.aa', 'A.bb', 'A.nn']], ['composeMulti', ['B.hh']]]);
      assert.deepEqual(calls.single, []); // nothing created, cleared, filled or loaded on the side
      assert.equal(calls.loadMany, 0);
      assert.deepEqual([calls.many[0].fills, calls.many[0].hasFill], [[7, 0, 2.5], [1, 0, 1]]);
      assert.deepEqual(calls.many[1].hasFill, [0]); // fillWith.h is falsy: no fill, as fillData was never called for it
      assert.deepEqual([calls.many[0].myLen, calls.many[0].hisLen, calls.many[1].hisLen], [[2, 2], [3, 4], [3, 2]]);
      assert.deepEqual(calls.many[0].maps, mapsOnto(cube, A));
      assert.deepEqual(calls.many[1].maps, mapsOnto(cube, B));
      assert.deepEqual([A.reshapes, B.reshapes], [1, 1]);
      assert.deepEqual(cube.storedMeasureIds, ['aa', 'bb', 'nn', 'hh']);
      assert.deepEqual(cube.storedMeasureIds.map((id) => cube.storedMeasures[id]._nativeStore.name),
                       ['composeMulti(A.aa)', 'composeMulti(A.bb)', 'composeMulti(A.nn)', 'composeMulti(B.hh)']);
      assert.deepEqual(cube.storedMeasureIds.map((id) => cube.storedMeasures[id]._type), ['float32', 'float64', 'int32', 'float32']);
      assert.deepEqual(cube.storedMeasuresRules.nn, { d1: 'sum', d2: 'sum' });
      assert.equal(HipStore.lastComposeCalls, 2);
      assert.equal(HipStore.lastBatchLaunches, 2);
    });
  });

  it('the old path reshapes and loads once per measure and makes no composeMulti', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    withStubbedAddon(calls, () => {
      const cube = A._composePerMeasure(B, false, { aa: 7 });
      assert.deepEqual([A.reshapes, B.reshapes], [3, 1]);
      assert.deepEqual(calls.many.map((c) => [c.op, c.targets.length]), [['loadMulti', 1], ['loadMulti', 2], ['loadMulti', 3], ['loadMulti', 1]]);
      assert.deepEqual(calls.single, ['fill new0 7']);
      assert.deepEqual(cube.storedMeasureIds, ['aa', 'bb', 'nn', 'hh']);
    });
  });

  it('a tracked measure keeps create + fill + load, once, and its place among the measures', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls, { bb: { orderTracked: 1 } }, { bb: { d1: 'last', d2: 'sum' } });
    withStubbedAddon(calls, () => {
      const cube = A.compose(B, true, { bb: 3 });
      assert.deepEqual(calls.many.map((c) => [c.op, c.sources]), [['composeMulti', ['A.aa', 'A.nn']], ['composeMulti', ['B.hh']]]);
      assert.deepEqual(calls.single, ['trackOrder new0', 'fill new0 3', 'load new0 <- A.bb']);
      assert.equal(calls.loadMany, 1); // once for A, never for B
      assert.deepEqual([A.reshapes, B.reshapes], [1, 1]);
      assert.deepEqual(cube.storedMeasureIds, ['aa', 'bb', 'nn', 'hh']);
      assert.equal(cube.storedMeasures.bb._nativeStore.name, 'new0');
      assert.equal(HipStore.lastComposeCalls, 2);
    });
  });

  it('a tracked source behind untracked rules is loaded the old way', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls, { aa: { orderTracked: 1 } });
    withStubbedAddon(calls, () => {
      A.compose(B);
      assert.deepEqual(calls.many.map((c) => [c.op, c.sources]), [['composeMulti', ['A.bb', 'A.nn']], ['loadMulti', ['A.aa']], ['composeMulti', ['B.hh']]]);
      assert.equal(calls.loadMany, 1);
      assert.equal(HipStore.lastComposeCalls, 2);
      assert.equal(HipStore.lastBatchLaunches, 3);
    });
  });

  it('measures split over devices take loadMany once per source and never composeMulti', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    withStubbedAddon(calls, () => {
      const cube = A.compose(B, false, { nn: 9 });
      assert.deepEqual(calls.many, []);
      assert.equal(calls.loadMany, 2);
      assert.deepEqual([A.reshapes, B.reshapes], [1, 1]);
      assert.deepEqual(calls.single.filter((c) => /^load /.test(c)),
                       ['load gather(sharded0) <- A.aa', 'load gather(sharded1) <- A.bb', 'load gather(sharded2) <- A.nn', 'load gather(sharded3) <- B.hh']);
      assert.deepEqual(calls.single.filter((c) => /^fill /.test(c)), ['fill sharded2 9']);
      assert.deepEqual(cube.storedMeasureIds, ['aa', 'bb', 'nn', 'hh']);
      assert.equal(HipStore.lastComposeCalls, 0);
    }, { world: 2 });
  });

  it('an addon without composeMulti keeps create + fill + load, loaded once per source', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    withStubbedAddon(calls, () => {
      const cube = A.compose(B, false, { bb: 4 });
      assert.deepEqual(calls.many.map((c) => [c.op, c.targets, c.sources]),
                       [['loadMulti', ['new0', 'new1', 'new2'], ['A.aa', 'A.bb', 'A.nn']], ['loadMulti', ['new3'], ['B.hh']]]);
      assert.deepEqual(calls.single, ['fill new1 4']);
      assert.deepEqual([A.reshapes, B.reshapes], [1, 1]);
      assert.deepEqual(cube.storedMeasureIds, ['aa', 'bb', 'nn', 'hh']);
      assert.equal(HipStore.lastComposeCalls, 0);
      assert.equal(HipStore.lastBatchLaunches, 2);
    }, { composeMulti: false });
  });

  it('cubes that cannot be brought together: the measures exist, filled, and nothing is loaded', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    A.reshape = () => { throw new Error("The cube dimensions 'd1' are not compatible."); };
    withStubbedAddon(calls, () => {
      const cube = A.compose(B, false, { aa: 7 });
      assert.deepEqual(calls.many.map((c) => [c.op, c.sources]), [['composeMulti', ['B.hh']]]);
      assert.deepEqual(calls.single, ['fill new0 7']);
      assert.equal(calls.loadMany, 0);
      assert.deepEqual(cube.storedMeasureIds.map((id) => cube.storedMeasures[id]._nativeStore.name), ['new0', 'new1', 'new2', 'composeMulti(B.hh)']);
      assert.equal(HipStore.lastComposeCalls, 1);
    });
  });

  it('a measure id in both cubes still throws', () => {
    const calls = newCalls();
    const A = stubCube('A', ['a', 'b'], ['x', 'y'], { aa: F32, bb: F64 }, calls);
    const B = stubCube('B', ['a', 'b'], ['x', 'y'], { hh: F32, bb: F64 }, calls);
    withStubbedAddon(calls, () => {
      assert.throws(() => A.compose(B), /This measure already exists: bb/);
      assert.throws(() => A._composePerMeasure(B), /This measure already exists: bb/);
    });
  });
});

describe('compose carries the computed measures of both cubes', () => {
  it('this first, otherCube overrides, on both paths', () => {
    const calls = newCalls();
    const [A, B] = twoCubes(calls);
    A.createComputedMeasure('margin', 'aa - bb');
    A.createComputedMeasure('twice', 'aa * 2');
    B.createComputedMeasure('margin', 'hh + 1');
    B.createComputedMeasure('half', 'hh / 2');
    withStubbedAddon(calls, () => {
      for (const cube of [A.compose(B), A._composePerMeasure(B)]) {
        assert.deepEqual(cube.computedMeasureIds, ['margin', 'twice', 'half']);
        assert.equal(cube.computedMeasures.margin, B.computedMeasures.margin);
        assert.equal(cube.computedMeasures.margin.toString(), B.computedMeasures.margin.toString());
        assert.equal(cube.computedMeasures.twice, A.computedMeasures.twice);
        assert.equal(cube.computedMeasures.half, B.computedMeasures.half);
      }
      assert.deepEqual(A.computedMeasureIds, ['margin', 'twice']); // the sources keep their own
      assert.ok(A.computedMeasures.margin !== B.computedMeasures.margin);
    });
  });
});

run();
