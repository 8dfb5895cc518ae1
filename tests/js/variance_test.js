'use strict';
/*
 * Cube.variance / Cube.stddev (dispersion roll-ups, one device call for the eligible measures) on the GPU: hand-worked
 * literals (the spread of a month's days on a daily TimeDimension, a GenericDimension whose region groups interleave),
 * then a seeded cube of mixed types, defaults and rules — `first` / `last` included — against the definition written
 * out on the host (Cube._varianceHost): data, status maps, totals, serialized bytes, rules; a computed measure over the
 * result; the source cube unchanged.  With a device list (OLAP_DEVICES) the measures are split over its devices and take
 * the host path.  (Every group here is far below the 1024 members from which the device may re-associate: the device
 * equals the definition bit for bit.)
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
  it('the spread of the days of a month on a daily dimension', () => {
    const cube = new Cube([new TimeDimension('time', 'day', '2010-01-01', '2010-02-28')]);
    cube.createStoredMeasure('revenue', { time: 'sum' }, 'float64', 0);
    cube.createStoredMeasure('small', { time: 'last' }, 'float32', 0);
    // January: 2 4 4 4 5 5 7 9 on its first eight days (mean 5, squared deviations 32), the rest unset;
    // February: 1001 .. 1004 on its last four days (mean 1002.5, squared deviations 5)
    const days = new Array(59).fill(0);
    [2, 4, 4, 4, 5, 5, 7, 9].forEach((v, d) => {
      days[d] = v;
    });
    [1001, 1002, 1003, 1004].forEach((v, d) => {
      days[55 + d] = v;
    });
    cube.setData('revenue', days);
    cube.setData('small', days);
    const variance = cube.variance('time', 'month');
    assert.deepEqual(variance.getData('revenue'), [4, 1.25]);
    assert.deepEqual(variance.getData('small'), [4, 1.25]);
    if (!SPLIT) assert.equal(HipStore.lastVariancePath, 'device');
    assert.deepEqual(variance.dimensions[0].getItems(), ['2010-01', '2010-02']);
    assert.deepEqual(variance.dimensions[0].getItems(), cube.drillUp('time', 'month').dimensions[0].getItems());
    assert.deepEqual(cube.stddev('time', 'month').getData('revenue'), [2, Math.sqrt(1.25)]);
    assert.deepEqual(cube.variance('time', 'month', 1).getData('revenue'), [32 / 7, 5 / 3]);
    assert.deepEqual(cube.variance('time', 'month', 1).getData('small'), [Math.fround(32 / 7), Math.fround(5 / 3)]);
    assert.deepEqual(cube.stddev('time', 'month', 1).getData('revenue'), [Math.sqrt(32 / 7), Math.sqrt(5 / 3)]);
    // twelve members as one group: sum 4050, mean 337.5
    const all = [2, 4, 4, 4, 5, 5, 7, 9, 1001, 1002, 1003, 1004];
    let m2 = 0;
    for (const v of all) m2 += (v - 337.5) * (v - 337.5);
    assert.deepEqual(cube.variance('time', 'all').getData('revenue'), [m2 / 12]);
    assert.deepEqual(cube.getData('revenue'), days); // the source cube is unchanged
    assert.ok(variance.storedMeasuresRules.revenue === cube.storedMeasuresRules.revenue);
    assert.ok(variance.storedMeasures.small.orderTracked && !variance.storedMeasures.revenue.orderTracked); // `last`: the order is kept from here on
    // the root attribute is not special: every day is a group of one member — 0, which is unset under the 0 default
    const byDay = cube.variance('time', 'day');
    assert.equal(byDay.getStatusMap('revenue').size, 0);
    assert.deepEqual(byDay.getData('revenue'), new Array(59).fill(0));
    assert.equal(cube.stddev('time', 'day', 1).getStatusMap('small').size, 0);
  });

  it('a GenericDimension whose region groups interleave, beside another dimension', () => {
    const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka', 'nice']);
    city.addAttribute('city', 'region', { paris: 'eu', tokyo: 'asia', lyon: 'eu', lima: 'america', osaka: 'asia', nice: 'eu' });
    const cube = new Cube([city, new GenericDimension('kind', 'kind', ['a', 'b'])]);
    cube.createStoredMeasure('num', { city: 'sum' }, 'float64', NaN_);
    cube.createStoredMeasure('mean', { city: 'average' }, 'float32', 0);
    cube.setNestedArray('num', [[1, 10], [2, 20], [NaN_, 30], [4, 40], [5, NaN_], [6, 60]]);
    cube.setNestedArray('mean', [[1, 10], [2, 20], [0, 30], [4, 40], [5, 0], [6, 60]]);
    const variance = cube.variance('city', 'region');
    // eu/a: 1, 6 (lyon unset): mean 3.5, 6.25; eu/b: 10, 30, 60: mean 100 / 3; asia/a: 2, 5: 2.25; asia/b: 20 alone; america: lima alone
    const mean = 100 / 3;
    const eubM2 = (10 - mean) * (10 - mean) + (30 - mean) * (30 - mean) + (60 - mean) * (60 - mean);
    const eub = eubM2 / 3;
    const regions = variance.dimensions[0].getItems();
    assert.deepEqual(regions.slice().sort(), ['america', 'asia', 'eu']);
    // one member: a SET 0 under the NaN default, unset (the default, 0) under the 0 default
    const want = { eu: [6.25, eub], asia: [2.25, 0], america: [0, 0] };
    assert.deepEqual(variance.getNestedArray('num'), regions.map((r) => want[r]));
    assert.deepEqual(variance.getNestedArray('mean'), regions.map((r) => want[r].map(Math.fround)));
    assert.equal(variance.getStatusMap('num').size, 6);
    assert.equal(variance.getStatusMap('mean').size, 3);
    // ddof 1: one member is unset whatever the default
    const sample = cube.stddev('city', 'region', 1);
    const wantSample = { eu: [Math.sqrt(12.5), Math.sqrt(eubM2 / 2)], asia: [Math.sqrt(4.5), NaN_], america: [NaN_, NaN_] };
    assert.deepEqual(sample.getNestedArray('num').map((row) => row.map((v) => (Number.isNaN(v) ? 'unset' : v))),
      regions.map((r) => wantSample[r].map((v) => (Number.isNaN(v) ? 'unset' : v))));
    assert.equal(sample.getStatusMap('num').size, 3);
    assert.deepEqual(cube.variance('kind', 'all').getNestedArray('num'), [[20.25], [81], [0], [324], [0], [729]]);
    // the root attribute: every set cell a group of one member, a SET 0 under the NaN default
    const byCity = cube.variance('city', 'city');
    assert.deepEqual(Array.from(byCity.getStatusMap('num').keys()).sort((x, y) => x - y), [0, 1, 2, 3, 5, 6, 7, 8, 10, 11]);
    assert.deepEqual(byCity.getData('num').filter((v) => !Number.isNaN(v)), new Array(10).fill(0));
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
      return type === 'float32' || type === 'float64' ? v + (next() < 0.3 ? 0.1 : 0) + (type === 'float64' && next() < 0.5 ? 1e9 : 0) : type === 'uint32' ? Math.abs(v) : v;
    });
    cube.setData(id, values);
  }
  return cube;
}

describe('against the definition written out on the host (_varianceHost)', () => {
  for (const [dimensionId, attribute, ddof, kind] of [['time', 'all', 0, 0], ['time', 'year', 1, 1], ['time', 'quarter', 0, 1], ['city', 'region', 1, 0],
    ['city', 'all', 0, 0], ['kind', 'all', 1, 1], ['time', 'semester', 0, 0], ['city', 'region', 0, 1], ['time', 'month', 0, 0]]) {
    it(`measures of mixed type, default and rule along ${dimensionId} by ${attribute}, ddof = ${ddof}, ${kind ? 'stddev' : 'variance'}`, () => {
      const cube = seededCube(true);
      const before = cube.storedMeasureIds.map((id) => cube.getData(id));
      const a = kind ? cube.stddev(dimensionId, attribute, ddof) : cube.variance(dimensionId, attribute, ddof);
      // the `first` / `last` measures are tracked and held on one device whatever the device list: they take the call
      assert.equal(HipStore.lastVariancePath, 'device');
      // one launch per (cell type, default): float32 / 0, float64 / NaN (integers are held in float64 cells too), float64 / 0, float32 / NaN
      if (!SPLIT) assert.equal(HipStore.lastBatchLaunches, 4);
      const b = cube._varianceHost(dimensionId, attribute, ddof, kind);
      assert.deepEqual(a.dimensionIds, b.dimensionIds);
      assert.deepEqual(a.dimensions.map((d) => d.getItems()), cube.drillUp(dimensionId, attribute).dimensions.map((d) => d.getItems()));
      assert.deepEqual(a.storedMeasureIds, b.storedMeasureIds);
      assert.deepEqual(a.storedMeasuresRules, b.storedMeasuresRules);
      for (const id of a.storedMeasureIds) {
        sameMeasure(a, b, id, `${dimensionId}/${attribute}/${ddof}/${kind}`);
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
    const a = cube.variance('time', 'year', 1);
    assert.equal(HipStore.lastVariancePath, SPLIT ? 'host' : 'device');
    if (!SPLIT) assert.equal(HipStore.lastBatchLaunches, 4);
    const b = cube._varianceHost('time', 'year', 1, 0);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'untracked');
    const s = cube.stddev('time', 'year', 1);
    assert.equal(HipStore.lastVariancePath, SPLIT ? 'host' : 'device');
    const t = cube._varianceHost('time', 'year', 1, 1);
    for (const id of a.storedMeasureIds) sameMeasure(s, t, id, 'untracked stddev');
  });

  it('eight measures of one type leave in one launch', () => {
    const cube = new Cube([new GenericDimension('d', 'item', ['p']), new TimeDimension('time', 'month', '2010-01', '2012-12')]);
    const next = rng(7);
    for (let k = 0; k < 8; ++k) {
      cube.createStoredMeasure(`m${k}`, { time: ['sum', 'average', 'highest', 'lowest', 'product'][k % 5] }, 'float32', 0);
      cube.setData(`m${k}`, Array.from({ length: cube.storeSize }, () => (next() < 0.25 ? 0 : Math.floor(next() * 9) - 3)));
    }
    const a = cube.stddev('time', 'year');
    assert.deepEqual([HipStore.lastVariancePath, HipStore.lastBatchLaunches], ['device', 1]); // (a first dimension of one item is never split)
    const b = cube._varianceHost('time', 'year', 0, 1);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'eight');
  });

  it('a computed measure over the result evaluates', () => {
    const cube = seededCube(false);
    cube.createComputedMeasure('double_revenue', 'revenue * 2 + low');
    const a = cube.stddev('time', 'year');
    const revenue = a.getData('revenue');
    const low = a.getData('low');
    assert.deepEqual(a.getData('double_revenue'), revenue.map((v, i) => v * 2 + low[i]));
    assert.deepEqual(a.computedMeasureIds, ['double_revenue']);
  });

  it('the errors', () => {
    const cube = seededCube(false);
    assert.throws(() => cube.variance('nowhere', 'all'), /variance: no such dimension: nowhere/);
    assert.throws(() => cube.stddev('time', 'fortnight'), /variance: no such attribute: fortnight/);
    assert.throws(() => cube.variance('time', 'year', 2), /variance: ddof must be 0 or 1/);
    assert.throws(() => cube.stddev('time', 'year', -1), /variance: ddof must be 0 or 1/);
    assert.throws(() => cube.variance('time', 'year', NaN_), /variance: ddof must be 0 or 1/);
    if (!SPLIT) {
      // no rule is consulted: a rule the seven-rule list refuses does not stop the call
      const ruled = seededCube(false);
      ruled.storedMeasuresRules.revenue = { time: 'median', city: 'sum', kind: 'sum' };
      assert.throws(() => ruled.drillUp('time', 'year'), /Unsupported aggregation method: median/);
      assert.equal(ruled.variance('time', 'year').getData('revenue').length, 3 * 3 * 7);
    }
  });
});

run();
