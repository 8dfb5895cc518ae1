'use strict';
/*
 * getTotalForDimensionItems / copyMeasureData of computed measures on the device (HipStore.selectTotalFormula /
 * copySelectFormula) against the per-cell methods (Cube._getTotalForDimensionItemsPerCell, _copyMeasureDataPerCell),
 * bit for bit: totals by Object.is, copies by serialize() bytes and getData of a twin cube.  Run plain and with
 * OLAP_DEVICES=0,0 (measures split over two shards: inputs are gathered, a sharded target copies cell by cell).
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, HipStore } = require('../../olap-in-memory_amd/js');

const sharded = !!process.env.OLAP_DEVICES;

function fixture() {
  const period = new GenericDimension('period', 'season', ['summer', 'winter']);
  const location = new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']);
  const cube = new Cube([location, period]);
  cube.createStoredMeasure('antennas', { period: 'sum', location: 'sum' }, 'uint32');
  cube.createStoredMeasure('routers', { period: 'sum', location: 'sum' }, 'uint32');
  cube.createComputedMeasure('router_by_antennas', 'routers / antennas');
  cube.setNestedArray('antennas', [[1, 2], [4, 8], [16, 32]]);
  cube.setNestedArray('routers', [[3, 2], [4, 9], [16, 32]]);
  return cube;
}

const FIXTURE_FILTERS = [{}, { location: 'paris' }, { period: ['winter', 'summer'] }, { period: 'summer', location: ['tokyo', 'paris', 'tokyo'] },
  { colour: ['red', 'blue'] }, { location: [] }, { location: undefined, period: 'winter' }];

let seed = 777;
const rnd = (n) => {
  seed = (seed * 1103515245 + 12345) % 2147483648;
  return Math.floor((seed / 2147483648) * n);
};
const TYPES = ['int32', 'uint32', 'float32', 'float64'];
// every opcode of the exact set (formula.js isDeviceExact), integer-valued over the random data below
const EXACT = ['m0 + m1', 'm1 - m2 * m3', 'm0 % 3 + -m2', 'm0 || m3', 'm1 ? m2 : m3', 'min(m0, m1, 2) + max(m2, m3)', 'isNaN(m3) + not m0',
  'abs(m2) + ceil(m3 / 4) - floor(m0 / 8) + trunc(m1 / 3)', 'sqrt(m1 * m1)', 'sign(m0 - m2)', 'if(m2, m0, 5)'];

function randomCube(s) {
  seed = s;
  const ndim = 1 + rnd(3);
  const dims = Array.from({ length: ndim }, (_, d) => new GenericDimension(`d${d}`, 'item', Array.from({ length: [1, 3, 5][rnd(3)] }, (_x, i) => `d${d}i${i}`)));
  const cube = new Cube(dims);
  TYPES.forEach((type, k) => {
    const def = rnd(2) ? Number.NaN : 0;
    cube.createStoredMeasure(`m${k}`, {}, type, def);
    cube.setData(`m${k}`, Array.from({ length: cube.storeSize }, () => (rnd(3) === 0 ? def : (rnd(40) - (type === 'uint32' ? 0 : 20)))));
  });
  EXACT.forEach((text, i) => cube.createComputedMeasure(`e${i}`, text));
  return cube;
}

function randomFilter(cube) {
  const filter = {};
  for (const id of cube.dimensionIds.slice().sort(() => rnd(3) - 1)) {
    if (rnd(2)) continue;
    const items = cube.getDimension(id).getItems();
    const list = Array.from({ length: rnd(items.length + 2) }, () => items[rnd(items.length)]);
    filter[id] = list.length === 1 && rnd(2) ? list[0] : list;
  }
  if (rnd(5) === 0) filter.extra = ['x', 'y'];
  return filter;
}

const bytes = (cube, m) => Buffer.from(cube.storedMeasures[m].serialize()).toString('hex');
// serialize() equality up to the sign and payload of NaN cells (V8's Math and x86 arithmetic may hand setValue a
// negative NaN where the device computes the positive one; DESIGN.md §7): the same indexes in the same order, the
// same values by Object.is
function sameBlob(a, b, m, msg) {
  if (bytes(a, m) === bytes(b, m)) return;
  const x = a.storedMeasures[m]._whole.toSparse();
  const y = b.storedMeasures[m]._whole.toSparse();
  assert.equal(Buffer.from(x.indexes.buffer).toString('hex'), Buffer.from(y.indexes.buffer).toString('hex'), msg);
  assert.equal(x.values.length, y.values.length, msg);
  x.values.forEach((v, i) => assert.ok(Object.is(v, y.values[i]), `${msg}: value ${i}: ${v} !== ${y.values[i]}`));
  assert.ok(Array.from(x.values).some(Number.isNaN), msg);
}
const same = (a, b, msg) => assert.ok(Object.is(a, b), `${msg}: ${a} !== ${b}`);

function deviceTotal(cube, m, f) {
  HipStore.lastSelectPath = null;
  const got = cube.getTotalForDimensionItems(m, f);
  const path = HipStore.lastSelectPath;
  same(got, cube._getTotalForDimensionItemsPerCell(m, f), `${m} ${JSON.stringify(f)}`);
  return path;
}

// copies `source` into `target` on the cube and on a twin with the per-cell loop; returns lastCopyPath
function checkCopy(make, source, target, f) {
  const a = make();
  const b = make();
  HipStore.lastCopyPath = null;
  a.copyMeasureData(source, target, f);
  const path = HipStore.lastCopyPath;
  b._copyMeasureDataPerCell(source, target, f);
  sameBlob(a, b, target, `${source} -> ${target} ${JSON.stringify(f)}`);
  assert.deepEqual(a.getData(target), b.getData(target));
  return path;
}

describe('getTotalForDimensionItems of computed measures', () => {
  it('fixture: router_by_antennas on the device, === per-cell', () => {
    const cube = fixture();
    for (const f of FIXTURE_FILTERS) assert.ok(deviceTotal(cube, 'router_by_antennas', f) !== null, JSON.stringify(f));
  });

  it('random cubes: every op of the exact set, all cell types and defaults, repeats, free keys, empty lists', () => {
    for (let s = 1; s <= 12; ++s) {
      const cube = randomCube(s);
      for (let t = 0; t < 4; ++t) {
        const f = randomFilter(cube);
        EXACT.forEach((_, i) => assert.ok(deviceTotal(cube, `e${i}`, f) !== null));
      }
    }
  });

  it('a pending dice as an input', () => {
    const cube = randomCube(99);
    const first = cube.dimensionIds[0];
    const items = cube.getDimension(first).getItems();
    const kept = items.length > 1 ? items.slice(1).reverse() : items;
    const diced = cube.dice(first, 'item', kept, true);
    for (const f of [{}, { [first]: [kept[0], kept[0]] }]) assert.equal(deviceTotal(diced, 'e0', f), 'device');
  });

  it('both certificate outcomes', () => {
    const cube = new Cube([new GenericDimension('key', 'item', ['a', 'b', 'c'])]);
    cube.createStoredMeasure('xx', {}, 'float64', 0);
    cube.createStoredMeasure('yy', {}, 'float64', 0);
    cube.setData('xx', [2 ** 53, 1, -(2 ** 53)]);
    cube.setData('yy', [0, 0, 0]);
    cube.createComputedMeasure('diff', 'xx - yy');
    cube.createComputedMeasure('third', 'xx / 3');
    cube.createComputedMeasure('whole', 'yy + 1');
    assert.equal(deviceTotal(cube, 'diff', {}), 'sequential');
    assert.equal(deviceTotal(cube, 'third', {}), 'sequential');
    assert.equal(deviceTotal(cube, 'whole', {}), 'device');
  });

  it('formulas outside the exact set stay per-cell', () => {
    const cube = fixture();
    cube.createComputedMeasure('rr', 'round(routers / 3)');
    cube.createComputedMeasure('pp', 'routers ^ 2');
    cube.createComputedMeasure('ss', 'sin(routers)');
    for (const m of ['rr', 'pp', 'ss']) assert.equal(deviceTotal(cube, m, { period: 'winter' }), null, m);
    cube.createComputedMeasure('tt', 'routers / routers__total');
    HipStore.lastSelectPath = null;
    let device;
    let perCell;
    try {
      cube.getTotalForDimensionItems('tt', {});
    } catch (e) {
      device = e.message;
    }
    try {
      cube._getTotalForDimensionItemsPerCell('tt', {});
    } catch (e) {
      perCell = e.message;
    }
    assert.ok(device !== undefined && device === perCell, `${device} / ${perCell}`);
    assert.equal(HipStore.lastSelectPath, null);
  });

  it('10^6 combinations of a two-input Float32 formula in under 2 s', () => {
    const cube = new Cube([new GenericDimension('da', 'item', Array.from({ length: 1000 }, (_, i) => `a${i}`)),
      new GenericDimension('db', 'item', Array.from({ length: 1000 }, (_, i) => `b${i}`))]);
    cube.createStoredMeasure('uu', {}, 'float32', 0);
    cube.createStoredMeasure('vv', {}, 'float32', 0);
    cube.setData('uu', Float32Array.from({ length: 1e6 }, (_, i) => i % 97));
    cube.setData('vv', Float32Array.from({ length: 1e6 }, (_, i) => 1 + (i % 13)));
    cube.createComputedMeasure('ww', 'uu * vv + 1');
    cube.createStoredMeasure('out', {}, 'float32', 0);
    const t0 = Date.now();
    const total = cube.getTotalForDimensionItems('ww', {});
    const t1 = Date.now();
    if (!sharded) cube.copyMeasureData('ww', 'out', {}); // (a sharded target copies cell by cell)
    const t2 = Date.now();
    let want = 0;
    for (let i = 0; i < 1e6; ++i) want += (i % 97) * (1 + (i % 13)) + 1;
    assert.equal(total, want);
    if (!sharded) assert.equal(cube.getSingleData('out', { da: 'a999', db: 'b999' }), (999999 % 97) * (1 + (999999 % 13)) + 1);
    assert.ok(t1 - t0 < 2000 && t2 - t1 < 2000, `total ${t1 - t0} ms, copy ${t2 - t1} ms`);
    console.log(`    10^6 combinations: total ${t1 - t0} ms, copy ${t2 - t1} ms`);
  });
});

describe('copyMeasureData from computed measures', () => {
  it('every target type and default, random filters', () => {
    for (let s = 1; s <= 8; ++s) {
      TYPES.forEach((type, k) => {
        const make = () => {
          const cube = randomCube(s);
          cube.createStoredMeasure('tt', {}, type, k % 2 ? Number.NaN : 0);
          return cube;
        };
        seed = 1000 * s + k;
        const f = randomFilter(make());
        const path = checkCopy(make, `e${(s + k) % EXACT.length}`, 'tt', f);
        if (!sharded && !Object.values(f).some((v) => Array.isArray(v) && v.length === 0)) assert.equal(path, 'device', JSON.stringify(f));
      });
    }
  });

  it('a tracked target keeps the per-cell key order', () => {
    const make = () => {
      const cube = randomCube(5);
      cube.createStoredMeasure('tt', { d0: 'last' }, 'float64', Number.NaN);
      cube.setSingleData('tt', Object.fromEntries(cube.dimensionIds.map((id) => [id, cube.getDimension(id).getItems().slice(-1)[0]])), 3);
      return cube;
    };
    const items = make().getDimension('d0').getItems();
    checkCopy(make, 'e0', 'tt', { d0: items.slice().reverse() });
    checkCopy(make, 'e3', 'tt', {});
  });

  it('the target as an input: device without revisits, per cell with repeats or free keys', () => {
    const cube = fixture();
    const make = () => fixture();
    assert.equal(checkCopy(make, 'router_by_antennas', 'antennas', { period: 'summer', location: ['tokyo', 'paris'] }), sharded ? null : 'device');
    assert.equal(checkCopy(make, 'router_by_antennas', 'antennas', {}), sharded ? null : 'device');
    assert.equal(checkCopy(make, 'router_by_antennas', 'antennas', { period: 'summer', location: ['tokyo', 'paris', 'tokyo'] }), null);
    assert.equal(checkCopy(make, 'router_by_antennas', 'routers', { colour: ['red', 'blue'] }), null);
    assert.equal(checkCopy(make, 'router_by_antennas', 'routers', { colour: ['red'] }), sharded ? null : 'device');
    assert.ok(cube);
  });

  it('formulas outside the exact set copy cell by cell', () => {
    const make = () => {
      const cube = fixture();
      cube.createComputedMeasure('rr', 'round(routers / 3)');
      cube.createStoredMeasure('tt', {}, 'float32', 0);
      return cube;
    };
    assert.equal(checkCopy(make, 'rr', 'tt', {}), null);
  });
});

run();
