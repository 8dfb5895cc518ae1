'use strict';
/*
 * Cube.cumulate (running aggregates along a dimension, one device call for the eligible measures) on the GPU:
 * hand-worked literals (year-to-date on a monthly TimeDimension, a GenericDimension whose region groups interleave),
 * then a seeded cube of mixed types and defaults against the definition run as written (Cube._cumulatePerItem: one
 * dice -> drillUp chain per item) — data, status maps, totals, serialized bytes, rules — a `last` measure on the
 * per-item path, a computed measure over the cumulated stores, and the source cube unchanged.
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
  it('year-to-date revenue on a 2-year monthly dimension', () => {
    const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2011-12')]);
    cube.createStoredMeasure('revenue', { time: 'sum' }, 'float32', 0);
    cube.createStoredMeasure('peak', { time: 'highest' }, 'int32', 0);
    //                       2010                                      2011
    const months = [1, 2, 0, 4, 0, 0, 7, -14, 9, 10, 0, 12, /**/ 0, 0, 3, 0, 5, 6, 0, 8, -22, 10, 11, 12];
    cube.setData('revenue', months);
    cube.setData('peak', months);
    const ytd = cube.cumulate('time', 'year');
    // an unset month carries the running value; 1+2+4+7-14 = 0 is unset and restarts; nothing set yet in 2011-01/02
    assert.deepEqual(ytd.getData('revenue'), [1, 3, 3, 7, 7, 7, 14, 0, 9, 19, 19, 31, /**/ 0, 0, 3, 3, 8, 14, 14, 22, 0, 10, 21, 33]);
    assert.deepEqual(ytd.getData('peak'), [1, 2, 2, 4, 4, 4, 7, 7, 9, 10, 10, 12, /**/ 0, 0, 3, 3, 5, 6, 6, 8, 8, 10, 11, 12]);
    assert.equal(ytd.getStatusMap('revenue').has(7), false);
    assert.equal(ytd.getStatusMap('revenue').has(12), false);
    assert.equal(ytd.getStatusMap('revenue').has(14), true);
    const all = cube.cumulate('time');
    assert.deepEqual(all.getData('revenue'), [1, 3, 3, 7, 7, 7, 14, 0, 9, 19, 19, 31, /**/ 31, 31, 34, 34, 39, 45, 45, 53, 31, 41, 52, 64]);
    if (!SPLIT) assert.equal(HipStore.lastCumulatePath, 'device');
    assert.deepEqual(cube.getData('revenue'), months); // the source cube is unchanged
    assert.deepEqual(ytd.dimensionIds, ['time']);
    assert.ok(ytd.storedMeasuresRules.revenue === cube.storedMeasuresRules.revenue);
  });

  it('a GenericDimension whose region groups interleave, beside another dimension', () => {
    const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka', 'nice']);
    city.addAttribute('city', 'region', { paris: 'eu', tokyo: 'asia', lyon: 'eu', lima: 'america', osaka: 'asia', nice: 'eu' });
    const cube = new Cube([city, new GenericDimension('kind', 'kind', ['a', 'b'])]);
    cube.createStoredMeasure('num', { city: 'sum' }, 'float64', NaN_);
    cube.createStoredMeasure('mean', { city: 'average' }, 'float32', 0);
    cube.setNestedArray('num', [[1, 10], [2, 20], [NaN_, 30], [4, 40], [5, NaN_], [6, 60]]);
    cube.setNestedArray('mean', [[1, 10], [2, 20], [0, 30], [4, 40], [5, 0], [6, 60]]);
    const running = cube.cumulate('city', 'region');
    //                                         paris     tokyo     lyon      lima      osaka     nice
    assert.deepEqual(running.getNestedArray('num'), [[1, 10], [2, 20], [1, 40], [4, 40], [7, 20], [7, 100]]);
    // contributions only: lyon/a is unset (1 / 1), osaka/b is unset (20 / 1), nice: (1 + 6) / 2 and (10 + 30 + 60) / 3
    assert.deepEqual(running.getNestedArray('mean'), [[1, 10], [2, 20], [1, 20], [4, 40], [3.5, 20], [3.5, 100 / 3].map(Math.fround)]);
    const kinds = cube.cumulate('kind');
    assert.deepEqual(kinds.getNestedArray('num'), [[1, 11], [2, 22], [NaN_, 30], [4, 44], [5, 5], [6, 66]]);
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

function seededCube(withLast) {
  const time = new TimeDimension('time', 'month', '2010-03', '2012-02');
  const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka', 'nice', 'quito']);
  city.addAttribute('city', 'region', { paris: 'eu', tokyo: 'asia', lyon: 'eu', lima: 'america', osaka: 'asia', nice: 'eu', quito: 'america' });
  const cube = new Cube([new GenericDimension('kind', 'kind', ['a', 'b', 'c']), time, city]);
  const next = rng(20240807);
  const kinds = [['revenue', 'sum', 'float32', 0], ['count', 'sum', 'int32', NaN_], ['mean', 'average', 'float64', NaN_], ['low', 'lowest', 'uint32', 0]];
  if (withLast) kinds.push(['latest', 'last', 'float32', 0]);
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

describe('against the definition run as written (_cumulatePerItem)', () => {
  for (const [dimensionId, attribute] of [['time', 'all'], ['time', 'year'], ['time', 'quarter'], ['city', 'region'], ['city', 'all'], ['kind', 'all']]) {
    it(`four measures of mixed type and default along ${dimensionId} by ${attribute}`, () => {
      const cube = seededCube(false);
      const before = cube.storedMeasureIds.map((id) => cube.getData(id));
      const a = cube.cumulate(dimensionId, attribute);
      if (!SPLIT) {
        assert.equal(HipStore.lastCumulatePath, 'device');
        // one launch per (cell type, default): float32 / 0, float64 / NaN (integers are held in float64 cells too), float64 / 0
        assert.equal(HipStore.lastBatchLaunches, 3);
      }
      const b = cube._cumulatePerItem(dimensionId, attribute);
      assert.deepEqual(a.dimensionIds, b.dimensionIds);
      assert.deepEqual(a.storedMeasureIds, b.storedMeasureIds);
      assert.deepEqual(a.storedMeasuresRules, b.storedMeasuresRules);
      for (const id of a.storedMeasureIds) {
        sameMeasure(a, b, id, `${dimensionId}/${attribute}`);
        assert.equal(a.storedMeasures[id]._type, b.storedMeasures[id]._type);
        assert.ok(Object.is(a.storedMeasures[id]._defaultValue, b.storedMeasures[id]._defaultValue));
      }
      assert.ok(Buffer.from(a.serialize()).equals(Buffer.from(b.serialize())), 'serialize()');
      cube.storedMeasureIds.forEach((id, i) => assert.deepEqual(cube.getData(id), before[i], `source ${id} changed`));
    });
  }

  it('a measure with a `last` rule takes the per-item path beside the device call, and matches', () => {
    const cube = seededCube(true);
    const a = cube.cumulate('time', 'year');
    if (!SPLIT) assert.equal(HipStore.lastCumulatePath, 'device');
    const b = cube._cumulatePerItem('time', 'year');
    assert.deepEqual(a.storedMeasureIds, ['revenue', 'count', 'mean', 'low', 'latest']);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'with last');
    // forward-fill: an unset cell of `latest` holds the last set value of its year so far
    const src = cube.getNestedArray('latest');
    const got = a.getNestedArray('latest');
    for (let m = 1; m < 10; ++m) if (src[0][m][0] === 0) assert.equal(got[0][m][0], got[0][m - 1][0]); // 2010-04 .. 2010-12
  });

  it('eight measures of one type leave in one launch', () => {
    const cube = new Cube([new GenericDimension('d', 'item', ['p', 'q', 'r']), new TimeDimension('time', 'month', '2010-01', '2012-12')]);
    const next = rng(7);
    for (let k = 0; k < 8; ++k) {
      cube.createStoredMeasure(`m${k}`, { time: ['sum', 'average', 'highest', 'lowest', 'product'][k % 5] }, 'float32', 0);
      cube.setData(`m${k}`, Array.from({ length: cube.storeSize }, () => (next() < 0.25 ? 0 : Math.floor(next() * 9) - 3)));
    }
    const a = cube.cumulate('time', 'year');
    if (!SPLIT) assert.deepEqual([HipStore.lastCumulatePath, HipStore.lastBatchLaunches], ['device', 1]);
    const b = cube._cumulatePerItem('time', 'year');
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'eight');
  });

  it('a computed measure over the cumulated stores evaluates', () => {
    const cube = seededCube(false);
    cube.createComputedMeasure('double_revenue', 'revenue * 2 + low');
    const a = cube.cumulate('time', 'year');
    const revenue = a.getData('revenue');
    const low = a.getData('low');
    assert.deepEqual(a.getData('double_revenue'), revenue.map((v, i) => v * 2 + low[i]));
    assert.deepEqual(a.computedMeasureIds, ['double_revenue']);
  });

  it('the errors, and the root attribute', () => {
    const cube = seededCube(false);
    assert.throws(() => cube.cumulate('nowhere'), /cumulate: no such dimension: nowhere/);
    assert.throws(() => cube.cumulate('time', 'fortnight'), /cumulate: no such attribute: fortnight/);
    const same = cube.cumulate('time', 'month');
    assert.ok(same !== cube);
    for (const id of cube.storedMeasureIds) sameMeasure(same, cube, id, 'root attribute');
  });
});

run();
