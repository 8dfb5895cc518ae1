'use strict';
/*
 * Cube.quantile / Cube.median (order-statistic roll-ups, one device call for the eligible measures) on the GPU:
 * hand-worked literals (the median day per month on a daily TimeDimension, a GenericDimension whose region groups
 * interleave), then a seeded cube of mixed types, defaults and rules — `first` / `last` included — against the
 * definition written out on the host (Cube._quantileHost): data, status maps, totals, serialized bytes, rules; a
 * computed measure over the result; the source cube unchanged.  With a device list (OLAP_DEVICES) the measures are
 * split over its devices and take the host path.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, HipStore } = require('../../olap-in-memory_amd/js');

const NaN_ = Number.NaN;
// a device list is set (OLAP_DEVICES): new measures are split over its devices wherever their first dimension allows
const SPLIT = HipStore.splits([1 << 20]);

function sameMeasure(a, b, id, where) {
  const x = a.getData(id);
  const y = b.getData(id);
  assert.equal(x.length, y.length, `${where}: ${id} size`);
  for (let i = 0; i < x.length; ++i) assert.ok(Object.is(x[i], y[i]), `${where}: ${id}[${i}] ${x[i]} !== ${y[i]}`);
  assert.deepEqual(Array.from(a.getStatusMap(id).entries()).sort((p, q) => p[0] - q[0]), Array.from(b.getStatusMap(id).entries()).sort((p, q) => p[0] - q[0]),
    `${where}: ${id} status map`);
  assert.ok(Object.is(a.getTotal(id), b.getTotal(id)), `${where}: ${id} total`);
}

describe('hand-worked literals', () => {
  it('the median day per month on a daily dimension', () => {
    const cube = new Cube([new TimeDimension('time', 'day', '2010-01-01', '2010-02-28')]);
    cube.createStoredMeasure('revenue', { time: 'sum' }, 'float32', 0);
    cube.createStoredMeasure('count', { time: 'last' }, 'int32', 0);
    // January: the day of the month, the 10th unset; February: 99 down to 72
    const days = [];
    for (let d = 1; d <= 31; ++d) days.push(d === 10 ? 0 : d);
    for (let d = 1; d <= 28; ++d) days.push(100 - d);
    cube.setData('revenue', days);
    cube.setData('count', days);
    const median = cube.median('time', 'month');
    // January: 30 members 1..9, 11..31, h = 14.5 between 16 and 17; February: 28 members 72..99, h = 13.5 between 85 and 86
    assert.deepEqual(median.getData('revenue'), [16.5, 85.5]);
    assert.deepEqual(median.dimensions[0].getItems(), ['2010-01', '2010-02']);
    assert.deepEqual(median.dimensions[0].getItems(), cube.drillUp('time', 'month').dimensions[0].getItems());
    // an integer measure is held in Float64 cells: its median keeps the half
    if (cube.storedMeasures.count._cells === 'float64') assert.deepEqual(median.getData('count'), [16.5, 85.5]);
    if (!SPLIT) assert.equal(HipStore.lastQuantilePath, 'device');
    assert.deepEqual(cube.quantile('time', 'month', 0.25).getData('revenue'), [8.25, 78.75]); // h = 7.25 between 8 and 9; h = 6.75 between 78 and 79
    assert.deepEqual(cube.quantile('time', 'month', 0).getData('revenue'), [1, 72]);
    assert.deepEqual(cube.quantile('time', 'month', 1).getData('revenue'), [31, 99]);
    assert.deepEqual(cube.median('time', 'all').getData('revenue'), [30.5]); // 58 members: 1..9, 11..31, 72..99; h = 28.5 between 30 and 31
    assert.deepEqual(cube.getData('revenue'), days); // the source cube is unchanged
    assert.ok(median.storedMeasuresRules.revenue === cube.storedMeasuresRules.revenue);
    assert.ok(median.storedMeasures.count.orderTracked && !median.storedMeasures.revenue.orderTracked); // `last`: the order is kept from here on
  });

  it('a GenericDimension whose region groups interleave, beside another dimension', () => {
    const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka', 'nice']);
    city.addAttribute('city', 'region', { paris: 'eu', tokyo: 'asia', lyon: 'eu', lima: 'america', osaka: 'asia', nice: 'eu' });
    const cube = new Cube([city, new GenericDimension('kind', 'kind', ['a', 'b'])]);
    cube.createStoredMeasure('num', { city: 'sum' }, 'float64', NaN_);
    cube.createStoredMeasure('mean', { city: 'average' }, 'float32', 0);
    cube.setNestedArray('num', [[1, 10], [2, 20], [NaN_, 30], [4, 40], [5, NaN_], [6, 60]]);
    cube.setNestedArray('mean', [[1, 10], [2, 20], [0, 30], [4, 40], [5, 0], [6, 60]]);
    const median = cube.median('city', 'region');
    const want = { eu: [3.5, 30], asia: [3.5, 20], america: [4, 40] }; // eu/a: 1, 6 (lyon unset); eu/b: 10, 30, 60; asia/a: 2, 5; asia/b: 20 (osaka unset)
    const regions = median.dimensions[0].getItems();
    assert.deepEqual(regions.slice().sort(), ['america', 'asia', 'eu']);
    assert.deepEqual(median.getNestedArray('num'), regions.map((r) => want[r]));
    assert.deepEqual(median.getNestedArray('mean'), regions.map((r) => want[r]));
    const low = { eu: [2.25, 20], asia: [2.75, 20], america: [4, 40] }; // q = 0.25: 1 + 0.25 * 5; 10 + 0.5 * 20; 2 + 0.25 * 3
    assert.deepEqual(cube.quantile('city', 'region', 0.25).getNestedArray('num'), regions.map((r) => low[r]));
    assert.deepEqual(cube.median('kind', 'all').getNestedArray('num'), [[5.5], [11], [30], [22], [5], [33]]);
    assert.deepEqual(cube.median('city', 'all').getNestedArray('mean'), [[4, 30]]); // a: 1 2 4 5 6; b: 10 20 30 40 60
    assert.deepEqual(cube.quantile('city', 'city', 0.9).getNestedArray('mean'), cube.getNestedArray('mean')); // the root attribute: a clone
  });
});

// mulberry32, as the other seeded tests
function rng(seed) {
  let a = seed >>> 0;
  return () => {
    a = (a + 0x6d2b79f5) >>> 0;
    let t = a;
    t = Math.imul(t ^ (t >>> 15), t | 1);
    t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
}

function seededCube(withOrdered) {
  const time = new TimeDimension('time', 'month', '2010-03', '2012-02');
  const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka', 'nice', 'quito']);
  city.addAttribute('city', 'region', { paris: 'eu', tokyo: 'asia', lyon: 'eu', lima: 'america', osaka: 'asia', nice: 'eu', quito: 'america' });
  const cube = new Cube([new GenericDimension('kind', 'kind', ['a', 'b', 'c']), time, city]);
  const next = rng(20240913);
  const kinds = [['revenue', 'sum', 'float32', 0], ['count', 'sum', 'int32', NaN_], ['mean', 'average', 'float64', NaN_], ['low', 'lowest', 'uint32', 0],
    ['ratio', 'product', 'float32', NaN_]];
  if (withOrdered) kinds.push(['opening', 'first', 'float64', 0], ['latest', 'last', 'float32', 0]);
  for (const [id, rule, type, def] of kinds) {
    cube.createStoredMeasure(id, { time: rule, city: rule, kind: rule }, type, def);
    const values = Array.from({ length: cube.storeSize }, () => {
      const u = next();
      if (u < 0.3) return def; // unset
      const v = Math.floor(next() * 13) - 4;
      return type === 'float32' || type === 'float64' ? v + (next() < 0.3 ? 0.1 : 0) : type === 'uint32' ? Math.abs(v) : v;
    });
    cube.setData(id, values);
  }
  return cube;
}

describe('against the definition written out on the host (_quantileHost)', () => {
  for (const [dimensionId, attribute, q] of [['time', 'all', 0.5], ['time', 'year', 0.9], ['time', 'quarter', 0.3], ['city', 'region', 0.5], ['city', 'all', 0.25],
    ['kind', 'all', 0.3], ['time', 'semester', 0], ['city', 'region', 1]]) {
    it(`measures of mixed type, default and rule along ${dimensionId} by ${attribute}, q = ${q}`, () => {
      const cube = seededCube(true);
      const before = cube.storedMeasureIds.map((id) => cube.getData(id));
      const a = cube.quantile(dimensionId, attribute, q);
      // the `first` / `last` measures are tracked and held on one device whatever the device list: they take the call
      assert.equal(HipStore.lastQuantilePath, 'device');
      // one launch per (cell type, default): float32 / 0, float64 / NaN (integers are held in float64 cells too), float64 / 0, float32 / NaN
      if (!SPLIT) assert.equal(HipStore.lastBatchLaunches, 4);
      const b = cube._quantileHost(dimensionId, attribute, q);
      assert.deepEqual(a.dimensionIds, b.dimensionIds);
      assert.deepEqual(a.dimensions.map((d) => d.getItems()), cube.drillUp(dimensionId, attribute).dimensions.map((d) => d.getItems()));
      assert.deepEqual(a.storedMeasureIds, b.storedMeasureIds);
      assert.deepEqual(a.storedMeasuresRules, b.storedMeasuresRules);
      for (const id of a.storedMeasureIds) {
        sameMeasure(a, b, id, `${dimensionId}/${attribute}/${q}`);
        assert.equal(a.storedMeasures[id]._type, b.storedMeasures[id]._type);
        assert.ok(Object.is(a.storedMeasures[id]._defaultValue, b.storedMeasures[id]._defaultValue));
        assert.equal(!!a.storedMeasures[id].orderTracked, !!b.storedMeasures[id].orderTracked, `${id} tracked`);
      }
      assert.ok(Buffer.from(a.serialize()).equals(Buffer.from(b.serialize())), 'serialize()');
      cube.storedMeasureIds.forEach((id, i) => assert.deepEqual(cube.getData(id), before[i], `source ${id} changed`));
    });
  }

  it('without tracked measures: the device on one device, the host under a device list', () => {
    const cube = seededCube(false);
    const a = cube.median('time', 'year');
    assert.equal(HipStore.lastQuantilePath, SPLIT ? 'host' : 'device');
    if (!SPLIT) assert.equal(HipStore.lastBatchLaunches, 4);
    const b = cube._quantileHost('time', 'year', 0.5);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'untracked');
    const m = cube.median('time', 'year');
    for (const id of a.storedMeasureIds) sameMeasure(a, m, id, 'median is quantile(0.5)');
  });

  it('eight measures of one type leave in one launch', () => {
    const cube = new Cube([new GenericDimension('d', 'item', ['p']), new TimeDimension('time', 'month', '2010-01', '2012-12')]);
    const next = rng(7);
    for (let k = 0; k < 8; ++k) {
      cube.createStoredMeasure(`m${k}`, { time: ['sum', 'average', 'highest', 'lowest', 'product'][k % 5] }, 'float32', 0);
      cube.setData(`m${k}`, Array.from({ length: cube.storeSize }, () => (next() < 0.25 ? 0 : Math.floor(next() * 9) - 3)));
    }
    const a = cube.quantile('time', 'year', 0.3);
    assert.deepEqual([HipStore.lastQuantilePath, HipStore.lastBatchLaunches], ['device', 1]); // (a first dimension of one item is never split)
    const b = cube._quantileHost('time', 'year', 0.3);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'eight');
  });

  it('a computed measure over the result evaluates', () => {
    const cube = seededCube(false);
    cube.createComputedMeasure('double_revenue', 'revenue * 2 + low');
    const a = cube.median('time', 'year');
    const revenue = a.getData('revenue');
    const low = a.getData('low');
    assert.deepEqual(a.getData('double_revenue'), revenue.map((v, i) => v * 2 + low[i]));
    assert.deepEqual(a.computedMeasureIds, ['double_revenue']);
  });

  it('the errors, and the root attribute', () => {
    const cube = seededCube(false);
    assert.throws(() => cube.quantile('nowhere', 'all', 0.5), /quantile: no such dimension: nowhere/);
    assert.throws(() => cube.median('time', 'fortnight'), /quantile: no such attribute: fortnight/);
    assert.throws(() => cube.quantile('time', 'year', 1.5), /quantile: q must lie in \[0, 1\]/);
    assert.throws(() => cube.quantile('time', 'year', NaN_), /quantile: q must lie in \[0, 1\]/);
    if (!SPLIT) {
      // `median` stays refused as a rule: the quantile is a call, not an eighth rule
      const ruled = seededCube(false);
      ruled.storedMeasuresRules.revenue = { time: 'median', city: 'sum', kind: 'sum' };
      assert.throws(() => ruled.drillUp('time', 'year'), /Unsupported aggregation method: median/);
      assert.equal(ruled.median('time', 'year').getData('revenue').length, 3 * 3 * 7);
    }
    const same = cube.quantile('time', 'month', 0.9);
    assert.ok(same !== cube);
    for (const id of cube.storedMeasureIds) sameMeasure(same, cube, id, 'root attribute');
  });
});

run();
