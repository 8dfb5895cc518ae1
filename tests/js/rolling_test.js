'use strict';
/*
 * Cube.rolling and Cube.shift (windows along a dimension, one device call for the eligible measures) on the GPU:
 * hand-worked literals on a monthly TimeDimension, then a seeded [4, 12, 5] cube with the months in the middle — Float32,
 * integer (held in Float64 cells) and float64 measures, and a `first` measure that goes item by item — against the
 * definition run as written (Cube._rollingPerItem: one dice -> drillUp chain per item): data, status maps, totals.
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
  it('trailing three months, a centred mean, last month and the same month a year ago', () => {
    const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2011-12')]);
    cube.createStoredMeasure('revenue', { time: 'sum' }, 'float32', 0);
    cube.createStoredMeasure('mean', { time: 'average' }, 'float64', NaN_);
    //                       2010                                      2011
    const months = [1, 2, 0, 4, 0, 0, 7, -7, 9, 10, 0, 12, /**/ 0, 0, 3, 0, 5, 6, 0, 8, -22, 10, 11, 12];
    cube.setData('revenue', months);
    cube.setData('mean', months.map((v) => (v === 0 ? NaN_ : v)));
    const trailing = cube.rolling('time', 2);
    // 7 - 7 = 0 is unset in 2010-08; every window starts afresh: 2010-09 is 7 - 7 + 9 with the restart inside the window
    assert.deepEqual(trailing.getData('revenue'), [1, 3, 3, 6, 4, 4, 7, 0, 9, 12, 19, 22, /**/ 12, 12, 3, 3, 8, 11, 11, 14, -14, -4, -1, 33]);
    assert.equal(trailing.getStatusMap('revenue').has(7), false);
    if (!SPLIT) assert.equal(HipStore.lastRollingPath, 'device');
    const ytd3 = cube.rolling('time', 2, 0, 'year');
    assert.deepEqual(ytd3.getData('revenue').slice(12, 15), [0, 0, 3]); // the window stops at the year
    const centred = cube.rolling('time', 1, 1);
    assert.deepEqual(centred.getData('mean').slice(0, 6), [1.5, 1.5, 3, 4, 4, 7]); // contributions only
    const lag = cube.shift('time', 1);
    assert.deepEqual(lag.getData('revenue'), [0].concat(months.slice(0, 23)));
    assert.deepEqual(cube.shift('time', 1, 'year').getData('revenue')[12], 0); // December is not in January's year
    const yearAgo = cube.shift('time', 12);
    assert.deepEqual(yearAgo.getData('revenue'), new Array(12).fill(0).concat(months.slice(0, 12)));
    const lead = cube.shift('time', -1, 'quarter');
    assert.deepEqual(lead.getData('revenue').slice(0, 6), [2, 0, 0, 0, 0, 0]); // 2010-03 and 2010-06 end their quarters
    assert.deepEqual(cube.getData('revenue'), months); // the source cube is unchanged
    assert.ok(trailing.storedMeasuresRules.revenue === cube.storedMeasuresRules.revenue);
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

function seededCube(lastMonth, withFirst) {
  const city = new GenericDimension('city', 'city', ['paris', 'tokyo', 'lyon', 'lima', 'osaka']);
  const cube = new Cube([new GenericDimension('kind', 'kind', ['a', 'b', 'c', 'd']), new TimeDimension('time', 'month', '2010-01', lastMonth), city]);
  const next = rng(20240915);
  const kinds = [['revenue', 'sum', 'float32', 0], ['cost', 'highest', 'float32', 0], ['count', 'sum', 'int32', NaN_], ['mean', 'average', 'float64', NaN_],
    ['low', 'lowest', 'uint32', 0]];
  if (withFirst) kinds.push(['opening', 'first', 'float32', 0]);
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

const CASES = [
  ['rolling(time, 2)', '2010-12', (c) => c.rolling('time', 2), (c, ids) => c._rollingPerItem('time', 2, 0, 'all', ids)],
  ['rolling(time, 11, 0, year)', '2010-12', (c) => c.rolling('time', 11, 0, 'year'), (c, ids) => c._rollingPerItem('time', 11, 0, 'year', ids)],
  ['rolling(time, 1, 1)', '2010-12', (c) => c.rolling('time', 1, 1), (c, ids) => c._rollingPerItem('time', 1, 1, 'all', ids)],
  ['shift(time, 1)', '2010-12', (c) => c.shift('time', 1), (c, ids) => c._rollingPerItem('time', 1, -1, 'all', ids)],
  ['shift(time, 12) over 24 months', '2011-12', (c) => c.shift('time', 12), (c, ids) => c._rollingPerItem('time', 12, -12, 'all', ids)],
  ['shift(time, -1, quarter)', '2010-12', (c) => c.shift('time', -1, 'quarter'), (c, ids) => c._rollingPerItem('time', -1, 1, 'quarter', ids)],
];

describe('against the definition run as written (_rollingPerItem)', () => {
  for (const [name, lastMonth, device, perItem] of CASES) {
    it(`${name}: five measures of mixed type and default, and a \`first\` measure item by item`, () => {
      const cube = seededCube(lastMonth, true);
      const before = cube.storedMeasureIds.map((id) => cube.getData(id));
      const a = device(cube);
      if (!SPLIT) {
        assert.equal(HipStore.lastRollingPath, 'device');
        // one launch per (cell type, default): float32 / 0 (two measures), float64 / NaN (integers are held in float64 cells too), float64 / 0
        assert.equal(HipStore.lastBatchLaunches, 3);
      }
      const b = perItem(cube, null);
      assert.deepEqual(a.dimensionIds, b.dimensionIds);
      assert.deepEqual(a.storedMeasureIds, ['revenue', 'cost', 'count', 'mean', 'low', 'opening']);
      assert.deepEqual(a.storedMeasureIds, b.storedMeasureIds);
      assert.deepEqual(a.storedMeasuresRules, b.storedMeasuresRules);
      for (const id of a.storedMeasureIds) {
        sameMeasure(a, b, id, name);
        assert.equal(a.storedMeasures[id]._type, b.storedMeasures[id]._type);
        assert.ok(Object.is(a.storedMeasures[id]._defaultValue, b.storedMeasures[id]._defaultValue));
      }
      cube.storedMeasureIds.forEach((id, i) => assert.deepEqual(cube.getData(id), before[i], `source ${id} changed`));
    });
  }

  it('eight measures of one type leave in one launch', () => {
    const cube = new Cube([new GenericDimension('d', 'item', ['p', 'q', 'r']), new TimeDimension('time', 'month', '2010-01', '2012-12')]);
    const next = rng(7);
    for (let k = 0; k < 8; ++k) {
      cube.createStoredMeasure(`m${k}`, { time: ['sum', 'average', 'highest', 'lowest', 'product'][k % 5] }, 'float32', 0);
      cube.setData(`m${k}`, Array.from({ length: cube.storeSize }, () => (next() < 0.25 ? 0 : Math.floor(next() * 9) - 3)));
    }
    const a = cube.rolling('time', 11, 0);
    if (!SPLIT) assert.deepEqual([HipStore.lastRollingPath, HipStore.lastBatchLaunches], ['device', 1]);
    const b = cube._rollingPerItem('time', 11, 0);
    for (const id of a.storedMeasureIds) sameMeasure(a, b, id, 'eight');
  });

  it('a computed measure of the result evaluates over the new stores', () => {
    const cube = seededCube('2010-12', false);
    cube.createComputedMeasure('double_revenue', 'revenue * 2 + low');
    const a = cube.rolling('time', 2);
    const revenue = a.getData('revenue');
    const low = a.getData('low');
    assert.deepEqual(a.getData('double_revenue'), revenue.map((v, i) => v * 2 + low[i]));
    assert.deepEqual(a.computedMeasureIds, ['double_revenue']);
    const growth = cube.shift('time', 1);
    assert.deepEqual(growth.getData('double_revenue'), growth.getData('revenue').map((v, i) => v * 2 + growth.getData('low')[i]));
  });

  it('the errors', () => {
    const cube = seededCube('2010-12', false);
    assert.throws(() => cube.rolling('nowhere', 1), /rolling: no such dimension: nowhere/);
    assert.throws(() => cube.rolling('time', 1, 0, 'fortnight'), /rolling: no such attribute: fortnight/);
    assert.throws(() => cube.rolling('time', 0.5), /rolling: before and after must be integers/);
    assert.throws(() => cube.rolling('time', 1, -2), /rolling: empty window/);
  });
});

run();
