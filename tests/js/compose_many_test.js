'use strict';
/*
 * Cube.compose with one device pass per source cube (HipStore.composeMany) against the reference's order of calls
 * (Cube._composePerMeasure: create, fill, hydrate, measure by measure): every compose case of gpu_test.js again with 1, 3
 * and 9 stored measures per cube of mixed types and defaults, some of them filled — the same data, status maps and
 * serialized bytes, and the hand-worked literals of those cases — then a tracked measure among sum measures, computed
 * measures on the composed cube, and what follows a compose.  Run plain and with OLAP_DEVICES=0,0 (measures split over
 * two shards keep the old calls).
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, HipStore, setCompactIntegers } = require('../../olap-in-memory_amd/js');

const NaN_ = Number.NaN;
const KINDS = [['float64', NaN_], ['int32', 0], ['float32', NaN_], ['uint32', 0], ['float64', 0], ['int32', NaN_], ['float32', 0], ['uint32', NaN_]];
const scaled = (data, f) => data.map((v) => (Array.isArray(v) ? scaled(v, f) : v * f));

/** `base` as the case declares it, then k - 1 more measures `<base>_<j>` holding j + 1 times the data, of mixed kinds */
function addMeasures(cube, base, data, def, k) {
  if (def === undefined) cube.createStoredMeasure(base);
  else cube.createStoredMeasure(base, {}, 'float32', def);
  cube.setNestedArray(base, data);
  for (let j = 1; j < k; ++j) {
    const [type, d] = KINDS[(j - 1) % KINDS.length];
    // (one measure keeps Int32 cells: it is loaded the old way, between cell types, among measures that are not)
    setCompactIntegers(j === 6);
    try {
      cube.createStoredMeasure(`${base}_${j}`, {}, type, d);
    } finally {
      setCompactIntegers(false);
    }
    cube.setNestedArray(`${base}_${j}`, scaled(data, j + 1));
  }
}

function pair(dims1, data1, dims2, data2, def, k) {
  const c1 = new Cube(dims1);
  const c2 = new Cube(dims2);
  addMeasures(c1, 'antennas', data1, def, k);
  addMeasures(c2, 'routers', data2, def, k);
  return [c1, c2];
}

function sameMeasure(a, b, id, where) {
  const x = a.getData(id);
  const y = b.getData(id);
  assert.equal(x.length, y.length, `${where}: ${id} size`);
  for (let i = 0; i < x.length; ++i) assert.ok(Object.is(x[i], y[i]), `${where}: ${id}[${i}] ${x[i]} !== ${y[i]}`);
  assert.deepEqual(Array.from(a.getStatusMap(id).entries()), Array.from(b.getStatusMap(id).entries()), `${where}: ${id} status map`);
}

// a device list is set (OLAP_DEVICES): new measures are split over its devices wherever their first dimension allows
const SPLIT = HipStore.splits([1 << 20]);

/** the composeMulti calls a compose of these two cubes makes: one per source with a measure that takes the pass */
function expectedCalls(composed, sources) {
  return sources.filter((cube) => cube.storedMeasureIds.some((id) => HipStore.composable(cube.storedMeasures[id]) &&
    !Object.values(cube.storedMeasuresRules[id] || {}).some((rule) => rule === 'first' || rule === 'last'))).length;
}

/** compose both ways; the new path must give what the old one gives, measure by measure */
function composed(c1, c2, union, fillWith, where) {
  const before = [c1, c2].map((cube) => cube.storedMeasureIds.map((id) => cube.getData(id)));
  const a = c1.compose(c2, union, fillWith);
  // (split measures keep the old calls; a composed cube too small to split takes the pass for what reshape left whole)
  if (SPLIT) assert.ok(HipStore.lastComposeCalls <= (HipStore.splits(a.dimensions.map((d) => d.numItems)) ? 0 : 2), `${where}: composeMulti calls`);
  else assert.equal(HipStore.lastComposeCalls, expectedCalls(a, [c1, c2]), `${where}: composeMulti calls`);
  const b = c1._composePerMeasure(c2, union, fillWith);
  assert.deepEqual(a.dimensionIds, b.dimensionIds);
  assert.deepEqual(a.storedMeasureIds, b.storedMeasureIds, `${where}: measure ids`);
  assert.deepEqual(a.storedMeasuresRules, b.storedMeasuresRules);
  for (const id of a.storedMeasureIds) {
    sameMeasure(a, b, id, where);
    assert.equal(a.storedMeasures[id]._type, b.storedMeasures[id]._type);
    assert.ok(Object.is(a.storedMeasures[id]._defaultValue, b.storedMeasures[id]._defaultValue));
  }
  assert.ok(Buffer.from(a.serialize()).equals(Buffer.from(b.serialize())), `${where}: serialize()`);
  [c1, c2].forEach((cube, c) => cube.storedMeasureIds.forEach((id, i) => assert.deepEqual(cube.getData(id), before[c][i], `${where}: source ${id} changed`)));
  return a;
}

// fills for some of the extra measures (the base measures keep the literals of gpu_test.js)
const fillsFor = (k) => (k >= 3 ? { antennas_1: 5, routers_2: 2.5, antennas_6: 4, routers_7: 9, antennas_3: 0 } : null);

for (const k of [1, 3, 9]) {
  describe(`compose (the cases of gpu_test.js) with ${k} stored measure(s) per cube`, () => {
    const period = () => new GenericDimension('period', 'season', ['summer', 'winter']);
    const cities = (items) => new GenericDimension('location', 'city', items);
    const grid = [[1, 2], [4, 8], [16, 32]];
    const both = (c1, c2, union, where) => {
      composed(c1, c2, union, fillsFor(k), `${where}, filled`);
      return composed(c1, c2, union, null, where);
    };
    for (const union of [false, true]) {
      const tag = union ? 'union' : 'intersection';
      const order = union ? ['paris', 'tokyo', 'toledo'] : ['paris', 'toledo', 'tokyo'];
      it(`${tag}: same dimensions`, () => {
        const loc = cities(order);
        const per = period();
        const [c1, c2] = pair([loc, per], grid, [loc, per], [[3, 2], [4, 9], [16, 32]], undefined, k);
        const c = both(c1, c2, union, tag);
        assert.deepEqual(c.dimensionIds, ['location', 'period']);
        assert.deepEqual(c.getNestedArray('routers'), [[3, 2], [4, 9], [16, 32]]);
        assert.deepEqual(c.getNestedArray('antennas'), grid);
        if (k >= 3) assert.deepEqual(c.getNestedArray('routers_2'), [[9, 6], [12, 27], [48, 96]]);
      });
      it(`${tag}: a dimension missing from one cube is summed away`, () => {
        const loc = cities(order);
        const [c1, c2] = pair([loc, period()], grid, [loc], [3, 4, 16], undefined, k);
        const c = both(c1, c2, union, tag);
        assert.deepEqual(c.dimensionIds, ['location']);
        assert.deepEqual(c.getNestedArray('antennas'), [3, 12, 48]);
        assert.deepEqual(c.getNestedArray('routers'), [3, 4, 16]);
        if (k >= 3) assert.deepEqual(c.getNestedArray('antennas_1'), [6, 24, 96]);
      });
      it(`${tag}: same time dimension`, () => {
        const time = new TimeDimension('time', 'month', '2010-01', '2010-02');
        const [c1, c2] = pair([time], [1, 2], [time], [3, 2], undefined, k);
        const c = both(c1, c2, union, tag);
        assert.deepEqual(c.dimensionIds, ['time']);
        assert.deepEqual(c.getNestedArray('antennas'), [1, 2]);
        assert.deepEqual(c.getNestedArray('routers'), [3, 2]);
      });
    }
    it('intersection: items missing from both cubes', () => {
      const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]], undefined, k);
      const c = both(c1, c2, false, 'missing items');
      assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [16, 32]]);
      assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [256, 512]]);
    });
    it('union: items missing from both cubes (NaN default), and the cells a fill reaches', () => {
      const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]], NaN_, k);
      const c = both(c1, c2, true, 'union, missing items');
      assert.deepEqual(c.getDimension('location').getItems(), ['paris', 'soria', 'tokyo', 'toledo']);
      assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [NaN_, NaN_], [16, 32], [4, 8]]);
      assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [64, 128], [256, 512], [NaN_, NaN_]]);
      if (k >= 3) {
        const filled = c1.compose(c2, true, fillsFor(k));
        assert.deepEqual(filled.getNestedArray('antennas_1'), [[2, 4], [5, 5], [32, 64], [8, 16]]); // float64 cells: soria is all fill
        assert.deepEqual(filled.getNestedArray('routers_2'), [[3072, 6144], [192, 384], [768, 1536], [2.5, 2.5]]); // int32 measure, Float64 cells
        assert.deepEqual(filled.getNestedArray('antennas'), [[1, 2], [NaN_, NaN_], [16, 32], [4, 8]]);
      }
    });
    it('overlapping time dimensions', () => {
      const t = (a, b, root = 'month') => new TimeDimension('time', root, a, b);
      let [c1, c2] = pair([t('2010-01', '2010-02')], [1, 2], [t('2010-02', '2010-03')], [3, 2], NaN_, k);
      assert.deepEqual(both(c1, c2, false, 'one common month').getNestedArray('antennas'), [2]);
      assert.deepEqual(c1.compose(c2).getNestedArray('routers'), [3]);
      assert.deepEqual(both(c1, c2, true, 'three months').getData('antennas'), [1, 2, NaN_]);
      assert.deepEqual(c1.compose(c2, true).getData('routers'), [NaN_, 3, 2]);
      [c1, c2] = pair([t('2010-01', '2010-02')], [1, 2], [t('2010-03', '2010-04')], [3, 2], NaN_, k);
      assert.equal(both(c1, c2, false, 'no common month').storeSize, 0);
      assert.deepEqual(both(c1, c2, true, 'four months').getData('antennas'), [1, 2, NaN_, NaN_]);
      assert.deepEqual(c1.compose(c2, true).getData('routers'), [NaN_, NaN_, 3, 2]);
      [c1, c2] = pair([t('2010-01', '2010-04')], [1, 2, 4, 8], [t('2010-Q1', '2010-Q3', 'quarter')], [16, 32, 64], undefined, k);
      assert.deepEqual(both(c1, c2, false, 'months and quarters').getNestedArray('antennas'), [7, 8]);
      assert.deepEqual(c1.compose(c2).getNestedArray('routers'), [16, 32]);
      [c1, c2] = pair([t('2010-01', '2010-04')], [1, 2, 4, 8], [t('2010-Q1', '2010-Q3', 'quarter')], [16, 32, 64], NaN_, k);
      assert.deepEqual(both(c1, c2, true, 'months and quarters, union').getData('antennas'), [7, 8, NaN_]);
      assert.deepEqual(c1.compose(c2, true).getData('routers'), [16, 32, 64]);
    });
    it('no common dimension: a single cell', () => {
      const [c1, c2] = pair([cities(['paris', 'toledo'])], [1, 2], [period()], [4, 8], undefined, k);
      const c = both(c1, c2, false, 'one cell');
      assert.deepEqual(c.dimensionIds, []);
      assert.deepEqual([c.getData('antennas'), c.getData('routers')], [[3], [12]]);
    });
  });
}

describe('a tracked measure among sum measures', () => {
  it('the sum measures leave in one composeMulti, the tracked one keeps its key order', () => {
    const build = (items) => {
      const cube = new Cube([new GenericDimension('location', 'city', items), new GenericDimension('period', 'season', ['summer', 'winter'])]);
      cube.createStoredMeasure('count', { location: 'sum', period: 'sum' }, 'float32', 0);
      cube.createStoredMeasure('latest', { location: 'last', period: 'last' }, 'float32', NaN_);
      cube.createStoredMeasure('weight', { location: 'sum', period: 'sum' }, 'float64', NaN_);
      return cube;
    };
    const c1 = build(['tokyo', 'paris', 'toledo']);
    // the tracked measure is written against the flat order: its keys come out in insertion order
    [[2, 1, 5], [0, 0, 6], [1, 1, 7], [0, 1, 8]].forEach(([l, p, v]) => c1.storedMeasures.latest.setValue(l * 2 + p, v));
    c1.setData('count', [1, 2, 3, 4, 5, 6]);
    c1.setData('weight', [0.5, NaN_, 1.5, 2.5, NaN_, 3.5]);
    const c2 = new Cube([new GenericDimension('location', 'city', ['paris', 'soria', 'tokyo']), new GenericDimension('period', 'season', ['summer', 'winter'])]);
    c2.createStoredMeasure('routers', {}, 'float32', 0);
    c2.setData('routers', [1, 2, 3, 4, 5, 6]);
    for (const union of [false, true]) {
      for (const fillWith of [null, { latest: 9, weight: 7 }]) {
        const where = `union ${union}, fill ${!!fillWith}`;
        const a = composed(c1, c2, union, fillWith, where);
        const b = c1._composePerMeasure(c2, union, fillWith);
        assert.deepEqual(Array.from(a.storedMeasures.latest._dataMap.keys()), Array.from(b.storedMeasures.latest._dataMap.keys()), `${where}: key order`);
        assert.deepEqual(a.storedMeasureIds, ['count', 'latest', 'weight', 'routers']);
        assert.ok(a.storedMeasures.latest.orderTracked && !a.storedMeasures.count.orderTracked);
        assert.deepEqual(a.drillUp('location', 'all').getData('latest'), b.drillUp('location', 'all').getData('latest'));
      }
    }
    c1.compose(c2);
    assert.equal(HipStore.lastComposeCalls, SPLIT ? 0 : 2);
  });
});

describe('computed measures travel with a compose', () => {
  const sales = () => {
    const cube = new Cube([new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']), new GenericDimension('period', 'season', ['summer', 'winter'])]);
    cube.createStoredMeasure('revenue', {}, 'float64', 0);
    cube.createStoredMeasure('cost', {}, 'float64', 0);
    cube.setNestedArray('revenue', [[10, 20], [30, 40], [50, 60]]);
    cube.setNestedArray('cost', [[1, 2], [3, 4], [5, 6]]);
    cube.createComputedMeasure('margin', 'revenue - cost');
    return cube;
  };
  const staff = () => {
    const cube = new Cube([new GenericDimension('location', 'city', ['tokyo', 'paris'])]);
    cube.createStoredMeasure('heads', {}, 'uint32', 0);
    cube.setNestedArray('heads', [5, 2]);
    cube.createComputedMeasure('pairs', 'heads / 2');
    return cube;
  };
  it('margin evaluates on the composed cube and equals the formula over the composed stored measures', () => {
    const c = sales().compose(staff());
    assert.deepEqual(c.dimensionIds, ['location']);
    assert.deepEqual(c.computedMeasureIds, ['margin', 'pairs']);
    assert.deepEqual(c.getNestedArray('revenue'), [30, 110]);
    assert.deepEqual(c.getNestedArray('cost'), [3, 11]);
    assert.deepEqual(c.getNestedArray('margin'), [27, 99]);
    assert.deepEqual(c.getData('margin'), c.getData('revenue').map((r, i) => r - c.getData('cost')[i]));
    assert.deepEqual(c.getNestedArray('pairs'), [1, 2.5]);
    c.createComputedMeasure('margin_per_head', 'margin / heads');
    assert.deepEqual(c.getNestedArray('margin_per_head'), [27 / 2, 99 / 5]);
    assert.deepEqual(sales()._composePerMeasure(staff()).getNestedArray('margin'), [27, 99]);
  });
  it('otherCube\'s formula wins on a clash; the sources keep theirs', () => {
    const a = sales();
    const b = staff();
    b.createComputedMeasure('margin', 'heads * 100');
    const c = a.compose(b);
    assert.deepEqual(c.getNestedArray('margin'), [200, 500]);
    assert.deepEqual(a.getNestedArray('margin'), [[9, 18], [27, 36], [45, 54]]);
    assert.deepEqual(b.getNestedArray('margin'), [500, 200]);
  });
});

describe('what follows a compose', () => {
  const loc = (items) => {
    const d = new GenericDimension('location', 'city', items);
    d.addAttribute('city', 'continent', { paris: 'europe', toledo: 'europe', tokyo: 'asia', soria: 'europe' });
    return d;
  };
  const period = () => new GenericDimension('period', 'season', ['summer', 'winter']);
  const cubes = () => {
    const c1 = new Cube([loc(['paris', 'toledo', 'tokyo']), period()]);
    addMeasures(c1, 'antennas', [[1, 2], [4, 8], [16, 32]], 0, 3);
    const c2 = new Cube([loc(['soria', 'tokyo', 'paris']), period()]);
    addMeasures(c2, 'routers', [[64, 128], [256, 512], [1024, 2048]], NaN_, 3);
    return [c1, c2];
  };
  it('drillUp and getNestedObject with totals equal the same calls on the old path\'s cube', () => {
    const [c1, c2] = cubes();
    for (const union of [false, true]) {
      const a = c1.compose(c2, union, { antennas_1: 5 });
      const b = c1._composePerMeasure(c2, union, { antennas_1: 5 });
      for (const id of a.storedMeasureIds) {
        assert.deepEqual(a.drillUp('location', 'continent').getNestedArray(id), b.drillUp('location', 'continent').getNestedArray(id), `${union} ${id} drillUp`);
        assert.deepEqual(a.getNestedObject(id, true), b.getNestedObject(id, true), `${union} ${id} totals`);
      }
    }
  });
  it('writing to the composed cube leaves the sources alone', () => {
    const [c1, c2] = cubes();
    const before = [c1.getData('antennas'), c1.getData('antennas_2'), c2.getData('routers')];
    const c = c1.compose(c2);
    const seen = c.getData('antennas');
    c.setSingleData('antennas', { location: 'paris', period: 'summer' }, 99);
    c.fillData('routers', 7);
    c.setData('antennas_2', c.getData('antennas_2').map(() => 1));
    assert.deepEqual([c1.getData('antennas'), c1.getData('antennas_2'), c2.getData('routers')], before);
    assert.deepEqual(c.getData('antennas'), [99].concat(seen.slice(1)));
    // and a second compose of the same cubes is not disturbed by the first one's cube
    assert.deepEqual(c1.compose(c2).getData('antennas'), seen);
  });
});

run();
