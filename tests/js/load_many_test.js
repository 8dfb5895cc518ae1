'use strict';
/*
 * hydrateFromCube, compose and project / reorderDimensions of cubes with SEVERAL stored measures whose cell types differ
 * between the two cubes (HipStore.loadMany / reorderMany: one device call, cells of another type converted on the device)
 * against cubes that hold ONE of the measures each, against a source re-declared in the target's types on the host, and
 * against literals worked out by hand from the reference's load (src/store/in-memory.js:139-176).  Run plain and with
 * OLAP_DEVICES=0,0 (measures split over two shards).
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, HipStore, setCompactIntegers } = require('../../olap-in-memory_amd/js');

const NaN_ = Number.NaN;
const G = (id, items) => new GenericDimension(id, 'item', items);

/** measures: [{ id, type, def, compact, data }] */
function build(dims, measures) {
  const cube = new Cube(dims);
  for (const m of measures) {
    setCompactIntegers(!!m.compact);
    try {
      cube.createStoredMeasure(m.id, {}, m.type, m.def);
    } finally {
      setCompactIntegers(false);
    }
    if (m.data) cube.setData(m.id, m.data);
  }
  return cube;
}

function sameMeasure(a, b, id, where) {
  const x = a.getData(id);
  const y = b.getData(id);
  assert.equal(x.length, y.length, `${where}: ${id} size`);
  for (let i = 0; i < x.length; ++i) assert.ok(Object.is(x[i], y[i]), `${where}: ${id}[${i}] ${x[i]} !== ${y[i]}`);
  assert.deepEqual(Array.from(a.getStatusMap(id).keys()), Array.from(b.getStatusMap(id).keys()), `${where}: ${id} keys`);
}

let seed = 77;
const rnd = (n) => {
  seed = (seed * 1103515245 + 12345) % 2147483648;
  return Math.floor((seed / 2147483648) * n);
};
const SHOWS = [0.1, -1.5, 0.4, 2 ** 24 + 1, 2 ** 31 + 5, -(2 ** 31) - 7, 1e40, -0];

function values(n, def, kind) {
  return Array.from({ length: n }, (_x, i) => {
    if (rnd(5) < 2) return def;
    if (kind === 'float64' && i < 2 * SHOWS.length) return SHOWS[i % SHOWS.length];
    if (kind === 'uint') return 1 + rnd(60);
    return rnd(60) - 5 || 7;
  });
}

describe('hydrateFromCube between cubes whose measures have other cell types', () => {
  const myDims = () => [G('d1', ['a', 'b', 'c']), G('d2', ['x', 'y', 'z', 'w'])];
  const hisDims = () => [G('d1', ['c', 'q', 'a']), G('d2', ['y', 'x', 'v'])]; // smaller; an extra and a missing item per dimension
  for (const [myDef, hisDef] of [[0, 0], [NaN_, 0], [0, NaN_], [NaN_, NaN_]]) {
    it(`four measures, my default ${myDef}, his default ${hisDef}: one device call, the same cells as measure by measure`, () => {
      seed = 1000 + (Number.isNaN(myDef) ? 1 : 0) + (Number.isNaN(hisDef) ? 2 : 0);
      const mine = [
        { id: 'mf', type: 'float64', def: myDef, data: values(12, myDef) },
        { id: 'md', type: 'float32', def: myDef, data: values(12, myDef) },
        { id: 'mi', type: 'float32', def: myDef, data: values(12, myDef) },
        { id: 'mc', type: 'int32', def: myDef, data: values(12, myDef) }, // Float64 cells
      ];
      const his = [
        { id: 'mf', type: 'float32', def: hisDef, data: values(9, hisDef) },
        { id: 'md', type: 'float64', def: hisDef, data: values(9, hisDef, 'float64') },
        { id: 'mi', type: 'int32', def: hisDef, data: values(9, hisDef) }, // Float64 cells
        { id: 'mc', type: 'int32', def: hisDef, compact: true, data: values(9, hisDef) }, // Int32 cells
        { id: 'only_his', type: 'float32', def: hisDef, data: values(9, hisDef) },
      ];
      const together = build(myDims(), mine);
      HipStore.lastLoadPath = null;
      together.hydrateFromCube(build(hisDims(), his));
      assert.equal(HipStore.lastLoadPath, 'device');
      // the source re-declared in MY types on the host, which leaves same-type loads
      const retyped = build(hisDims(), his.slice(0, 4).map((m, k) => Object.assign({}, m, { type: mine[k].type, compact: false, data: null })));
      const source = build(hisDims(), his);
      for (const m of mine) retyped.setData(m.id, source.getData(m.id));
      const viaHost = build(myDims(), mine);
      viaHost.hydrateFromCube(retyped);
      for (let k = 0; k < mine.length; ++k) {
        const single = build(myDims(), [mine[k]]);
        single.hydrateFromCube(build(hisDims(), [his[k]]));
        sameMeasure(together, single, mine[k].id, 'one measure per cube');
        sameMeasure(together, viaHost, mine[k].id, 'source re-declared on the host');
      }
    });
  }

  it('2 x 3 by hand: a float64 source under NaN into float32 cells under 0', () => {
    // his (b, z) = 0.5 and (b, x) = NaN (unset: getValue hands out his default NaN, which my setValue keeps: NaN !== 0);
    // item q is not mine
    const mine = build([G('d1', ['a', 'b']), G('d2', ['x', 'y', 'z'])], [{ id: 'mm', type: 'float32', def: 0, data: [1, 2, 3, 4, 5, 6] }]);
    const his = build([G('d1', ['b', 'q']), G('d2', ['z', 'x'])], [{ id: 'mm', type: 'float64', def: NaN_, data: [0.5, NaN_, 7, 8] }]);
    mine.hydrateFromCube(his);
    assert.deepEqual(mine.getData('mm'), [1, 2, 3, NaN_, 5, 0.5]);
    assert.deepEqual(Array.from(mine.getStatusMap('mm').keys()), [0, 1, 2, 3, 4, 5]);
    assert.equal(HipStore.lastLoadPath, 'device');
  });

  it('2 x 3 by hand: compact int32 cells under NaN into float32 cells under NaN, and 0.1 from float64 rounds to float32', () => {
    // his unset (b, x) hands out NaN, which under MY NaN default deletes my cell
    const mine = build([G('d1', ['a', 'b']), G('d2', ['x', 'y', 'z'])], [{ id: 'mm', type: 'float32', def: NaN_, data: [1, 2, 3, 4, 5, 6] },
      { id: 'rr', type: 'float32', def: 0, data: [1, 2, 3, 4, 5, 6] }]);
    const his = build([G('d1', ['b', 'q']), G('d2', ['z', 'x'])], [{ id: 'mm', type: 'int32', def: NaN_, compact: true, data: [3, NaN_, 7, 8] },
      { id: 'rr', type: 'float64', def: 0, data: [0.1, 0, 7, 8] }]);
    mine.hydrateFromCube(his);
    assert.deepEqual(mine.getData('mm'), [1, 2, 3, NaN_, 5, 3]);
    assert.deepEqual(Array.from(mine.getStatusMap('mm').keys()), [0, 1, 2, 4, 5]);
    // his (b, x) = 0 is his default and mine: my cell is deleted
    assert.deepEqual(mine.getData('rr'), [1, 2, 3, 0, 5, Math.fround(0.1)]);
    assert.deepEqual(Array.from(mine.getStatusMap('rr').keys()), [0, 1, 2, 4, 5]);
  });
});

describe('compose of cubes whose measures differ in type', () => {
  const cities = (items) => new GenericDimension('location', 'city', items);
  const period = () => new GenericDimension('period', 'season', ['summer', 'winter']);
  const grid = [[1, 2], [4, 8], [16, 32]];
  // antennas in Float32 cells, routers declared int32 in compact Int32 cells; the composed cube is made without
  // setCompactIntegers, so its routers live in Float64 cells and every hydrateFromCube of them loads across cell types
  function pair(dims1, data1, dims2, data2, def) {
    const c1 = build(dims1, [{ id: 'antennas', type: 'float32', def }]);
    const c2 = build(dims2, [{ id: 'routers', type: 'int32', def, compact: true }]);
    c1.setNestedArray('antennas', data1);
    c2.setNestedArray('routers', data2);
    return [c1, c2];
  }
  it('union: items missing from both cubes (NaN default)', () => {
    const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]], NaN_);
    HipStore.lastLoadPath = null;
    const c = c1.compose(c2, true);
    assert.equal(HipStore.lastLoadPath, 'device');
    assert.equal(c.storedMeasures.routers._cells, 'float64');
    assert.equal(c2.storedMeasures.routers._cells, 'int32');
    assert.deepEqual(c.getDimension('location').getItems(), ['paris', 'soria', 'tokyo', 'toledo']);
    assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [NaN_, NaN_], [16, 32], [4, 8]]);
    assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [64, 128], [256, 512], [NaN_, NaN_]]);
  });
  it('intersection: items missing from both cubes', () => {
    const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]], NaN_);
    const c = c1.compose(c2);
    assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [16, 32]]);
    assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [256, 512]]);
  });
  it('union under a 0 default: same dimensions, and a dimension missing from one cube is summed away', () => {
    const order = ['paris', 'tokyo', 'toledo'];
    let [c1, c2] = pair([cities(order), period()], grid, [cities(order), period()], [[3, 2], [4, 9], [16, 32]], 0);
    let c = c1.compose(c2, true);
    assert.deepEqual(c.getNestedArray('routers'), [[3, 2], [4, 9], [16, 32]]);
    assert.deepEqual(c.getNestedArray('antennas'), grid);
    [c1, c2] = pair([cities(order), period()], grid, [cities(order)], [3, 4, 16], 0);
    c = c1.compose(c2, true);
    assert.deepEqual(c.dimensionIds, ['location']);
    assert.deepEqual(c.getNestedArray('antennas'), [3, 12, 48]);
    assert.deepEqual(c.getNestedArray('routers'), [3, 4, 16]);
  });
});

describe('project / reorderDimensions of four measures', () => {
  const dims = () => [new TimeDimension('t', 'quarter', '2010-Q1', '2010-Q4'), G('d1', ['a', 'b', 'c', 'd', 'e', 'f']), G('d2', Array.from({ length: 10 }, (_x, i) => `i${i}`))];
  seed = 31;
  const measures = [
    { id: 'm0', type: 'float32', def: 0, data: values(240, 0) },
    { id: 'm1', type: 'float32', def: 0, data: values(240, 0) },
    { id: 'm2', type: 'float64', def: NaN_, data: values(240, NaN_, 'float64') },
    { id: 'm3', type: 'int32', def: NaN_, compact: true, data: values(240, NaN_) },
  ];
  for (const [name, chain] of [
    ['reorderDimensions [d2, t, d1]', (c) => c.reorderDimensions(['d2', 't', 'd1'])],
    ['swapDimensions(t, d1)', (c) => c.swapDimensions('t', 'd1')],
    ['project [d2, t]', (c) => c.project(['d2', 't'])],
    ['dice -> reorderDimensions', (c) => c.dice('d1', 'item', ['e', 'b'], true).reorderDimensions(['d1', 'd2', 't'])],
  ]) {
    it(name, () => {
      const multi = chain(build(dims(), measures));
      for (const m of measures) sameMeasure(multi, chain(build(dims(), [m])), m.id, name);
    });
  }
});

run();
