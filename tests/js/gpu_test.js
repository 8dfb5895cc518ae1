'use strict';
/*
 * Cube-level parity on the GPU through the Node.js host + N-API addon.  Inputs and expected
 * values are the known-answer data of the reference's own tests (test/cube-accessors.js,
 * cube-drilling.js, cube-filtering.js, cube-dimension.js, cube-to-cube.js:403-606, fixture
 * test/helpers/create-test-cube.js:4-57), re-expressed for this harness, plus BASELINE config 1
 * against the reference's recorded output (tests/golden/configs.json).
 */
const fs = require('fs');
const path = require('path');
const { describe, it, beforeEach, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension } = require('../../olap-in-memory_amd/js');

const NaN_ = Number.NaN;

function testCube(fill = true) {
  const period = new GenericDimension('period', 'season', ['summer', 'winter']);
  const location = new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']);
  location.addAttribute('city', 'country', { paris: 'france', toledo: 'spain', tokyo: 'japan' });
  location.addAttribute('city', 'continent', { paris: 'europe', toledo: 'europe', tokyo: 'asia' });
  location.addAttribute('city', 'citySize', { paris: 'big', toledo: 'small', tokyo: 'big' });
  const cube = new Cube([location, period]);
  cube.createStoredMeasure('antennas', { period: 'sum', location: 'sum' }, 'uint32');
  cube.createStoredMeasure('routers', { period: 'sum', location: 'sum' }, 'uint32');
  if (fill) {
    cube.setNestedArray('antennas', [[1, 2], [4, 8], [16, 32]]);
    cube.setNestedArray('routers', [[3, 2], [4, 9], [16, 32]]);
  }
  return cube;
}

describe('accessors', () => {
  let cube;
  beforeEach(() => {
    cube = testCube();
  });
  it('sizes', () => {
    assert.equal(cube.storeSize, 6);
    assert.equal(cube.byteLength, 48);
  });
  it('flat, nested array, nested object, totals', () => {
    assert.deepEqual(cube.getData('antennas'), [1, 2, 4, 8, 16, 32]);
    assert.deepEqual(cube.getNestedArray('antennas'), [[1, 2], [4, 8], [16, 32]]);
    assert.deepEqual(cube.getNestedObject('antennas'), { paris: { summer: 1, winter: 2 }, toledo: { summer: 4, winter: 8 }, tokyo: { summer: 16, winter: 32 } });
    assert.deepEqual(cube.getNestedObject('antennas', true), {
      paris: { summer: 1, winter: 2, all: 3 },
      toledo: { summer: 4, winter: 8, all: 12 },
      tokyo: { summer: 16, winter: 32, all: 48 },
      all: { summer: 21, winter: 42, all: 63 },
    });
    assert.equal(cube.getTotal('antennas'), 63);
    assert.equal(cube.getSingleData('antennas', { location: 'toledo', period: 'winter' }), 8);
  });
  it('zero-dimension cube with totals', () => {
    const c = new Cube([]);
    c.createStoredMeasure('antennas');
    c.setData('antennas', [32]);
    assert.deepEqual(c.getNestedObject('antennas', true), 32);
  });
  it('setters', () => {
    const c = testCube(false);
    c.setData('antennas', [1, 2, 4, 8, 16, 32]);
    assert.deepEqual(c.getData('antennas'), [1, 2, 4, 8, 16, 32]);
    c.setNestedObject('routers', { paris: { summer: 1, winter: 2 }, toledo: { summer: 4, winter: 8 }, tokyo: { summer: 16, winter: 32 } });
    assert.deepEqual(c.getData('routers'), [1, 2, 4, 8, 16, 32]);
    assert.throws(() => c.setData('antennas', [1, 2, 3]), /value length is invalid: 6 !== 3/);
  });
  it('hydrateFromSparseNestedObject, null unsets', () => {
    const c = new Cube([new GenericDimension('period', 'season', ['summer', 'winter']), new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo'])]);
    c.createStoredMeasure('antennas', {}, 'float32', 0);
    c.hydrateFromSparseNestedObject('antennas', { winter: { toledo: 1, losangeles: 2 } });
    assert.deepEqual(c.getNestedObject('antennas'), { summer: { paris: 0, toledo: 0, tokyo: 0 }, winter: { paris: 0, toledo: 1, tokyo: 0 } });
    cube.hydrateFromSparseNestedObject('antennas', { toledo: { summer: null } });
    assert.equal(cube.getData('antennas')[2], 0);
    assert.equal(cube.getStatusMap('antennas').get(2), undefined);
    assert.deepEqual(Array.from(cube.getStatusMap('antennas').keys()), [0, 1, 3, 4, 5]);
  });
});

describe('drillUp', () => {
  it('no-op returns this', () => {
    const cube = testCube();
    assert.equal(cube.drillUp('location', 'city'), cube);
  });
  it('cities to continents', () => {
    assert.deepEqual(testCube().drillUp('location', 'continent').getNestedArray('antennas'), [[5, 10], [16, 32]]);
  });
  it('incomplete time cube, NaN default: sum and average with totals', () => {
    const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-06')]);
    cube.createStoredMeasure('data_sum', {}, 'float32', NaN_);
    cube.createStoredMeasure('data_avg', { time: 'average' }, 'float32', NaN_);
    cube.hydrateFromSparseNestedObject('data_sum', { '2010-01': 1, '2010-03': 2 });
    cube.hydrateFromSparseNestedObject('data_avg', { '2010-01': 10, '2010-02': 0, '2010-03': 20 });
    const up = cube.drillUp('time', 'quarter');
    assert.deepEqual(up.getNestedObject('data_sum', true), { '2010-Q1': 3, '2010-Q2': NaN_, all: 3 });
    assert.deepEqual(up.getNestedObject('data_avg', true), { '2010-Q1': 10, '2010-Q2': NaN_, all: 10 });
  });
  it('unknown method', () => {
    const cube = testCube();
    cube.updateStoredMeasureRules('antennas', () => ({ location: 'median' }));
    assert.throws(() => cube.drillUp('location', 'continent'), /Unsupported aggregation method: median/);
  });
});

describe('drillDown', () => {
  it('no-op returns this', () => {
    const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-02')]);
    cube.createStoredMeasure('measure1', { time: 'sum' }, 'float32');
    cube.setNestedObject('measure1', { '2010-01': 100, '2010-02': 100 });
    assert.equal(cube.drillDown('time', 'month'), cube);
  });
  for (const [root, start, end] of [['month', '2010-01', '2010-02'], ['month_week_mon', '2010-01-W1-mon', '2010-02-W1-mon']]) {
    it(`${root} -> day -> ${root} round trip (uint32 sum and average)`, () => {
      const cube = new Cube([new TimeDimension('time', root, start, end)]);
      cube.createStoredMeasure('measure1', { time: 'sum' }, 'uint32');
      cube.createStoredMeasure('measure2', { time: 'average' }, 'uint32');
      cube.setNestedObject('measure1', { [start]: 100, [end]: 100 });
      cube.setNestedObject('measure2', { [start]: 100, [end]: 100 });
      const days = cube.drillDown('time', 'day');
      assert.deepEqual(days.drillUp('time', root).getNestedObject('measure1'), cube.getNestedObject('measure1'));
      assert.deepEqual(days.drillUp('time', root).getNestedObject('measure2'), cube.getNestedObject('measure2'));
      if (root === 'month') {
        // integer remainder spreading: 100 over 31 days -> 7 days get 4, the rest 3
        const jan = days.getData('measure1').slice(0, 31);
        assert.equal(jan.reduce((a, b) => a + b, 0), 100);
        assert.deepEqual(Array.from(new Set(jan)).sort(), [3, 4]);
      }
    });
  }
  it('quarter to month, incomplete cube', () => {
    const cube = new Cube([new TimeDimension('time', 'quarter', '2010-Q1', '2010-Q2')]);
    cube.createStoredMeasure('measure1', { time: 'sum' }, 'float32', NaN_);
    cube.hydrateFromSparseNestedObject('measure1', { '2010-Q1': 90 });
    const months = cube.drillDown('time', 'month');
    assert.deepEqual(cube.getData('measure1'), [90, NaN_]);
    assert.deepEqual(months.drillUp('time', 'quarter').getData('measure1'), [90, NaN_]);
    assert.deepEqual(months.getData('measure1'), [30, 30, 30, NaN_, NaN_, NaN_]);
    assert.deepEqual(Array.from(months.getStatusMap('measure1').keys()), [0, 1, 2]);
  });
});

describe('slice and dice', () => {
  let cube;
  beforeEach(() => {
    cube = testCube();
  });
  it('slice', () => {
    const paris = cube.slice('location', 'city', 'paris');
    assert.deepEqual(paris.getNestedArray('antennas'), [1, 2]);
    assert.equal(paris.dimensions.length, 1);
    assert.equal(paris.dimensions[0].id, 'period');
    const winter = cube.slice('period', 'season', 'winter');
    assert.deepEqual(winter.getNestedArray('antennas'), [2, 8, 32]);
    assert.equal(winter.dimensions[0].id, 'location');
    assert.deepEqual(winter.slice('location', 'city', 'toledo').getNestedArray('antennas'), 8);
    const none = cube.slice('period', 'all', 'all').slice('location', 'all', 'all');
    assert.deepEqual(none.getNestedArray('antennas'), 63);
    assert.equal(none.dimensions.length, 0);
    assert.deepEqual(cube.collapse().getNestedArray('routers'), 66);
  });
  it('dice', () => {
    assert.equal(cube.dice('location', 'city', ['paris', 'toledo', 'tokyo']), cube);
    assert.deepEqual(cube.dice('location', 'city', ['paris', 'toledo']).getNestedArray('antennas'), [[1, 2], [4, 8]]);
    assert.deepEqual(cube.dice('location', 'city', ['toledo', 'paris']).getNestedArray('antennas'), [[1, 2], [4, 8]]);
    assert.deepEqual(cube.dice('location', 'continent', ['europe']).getNestedArray('antennas'), [[1, 2], [4, 8]]);
    assert.deepEqual(cube.dice('period', 'season', ['winter']).getNestedArray('antennas'), [[2], [8], [32]]);
    assert.equal(cube.dice('location', 'city', ['nonexisting', 'paris']).storeSize, cube.storeSize / 3);
    assert.equal(cube.dice('location', 'city', []).storeSize, 0);
    assert.deepEqual(cube.dice('location', 'city', ['toledo', 'paris'], true).getNestedArray('antennas'), [[4, 8], [1, 2]]);
    assert.throws(() => cube.dice('location', 'continent', ['europe'], true));
    assert.deepEqual(cube.diceByDimensionItems({ location: ['tokyo'], period: 'summer' }).getNestedArray('antennas'), [[16]]);
  });
});

describe('pending dice (fused dice -> drillUp)', () => {
  it('composes selections and fuses with the following drillUp', () => {
    const cube = testCube();
    const diced = cube.dice('location', 'city', ['tokyo', 'paris'], true); // reordered: [[16,32],[1,2]]
    assert.ok(diced.storedMeasures.antennas._pending, 'dice is lazy');
    const twice = diced.dice('location', 'city', ['paris']); // [[1,2]]
    assert.ok(twice.storedMeasures.antennas._pending, 'dice of a dice is still lazy');
    assert.deepEqual(twice.drillUp('period', 'all').getNestedArray('antennas'), [[3]]);
    assert.ok(twice.storedMeasures.antennas._pending, 'the fused drillUp did not materialise the dice');
    assert.deepEqual(twice.getNestedArray('antennas'), [[1, 2]]);
    assert.ok(!twice.storedMeasures.antennas._pending, 'reading cells materialises');
    assert.deepEqual(diced.removeDimension('location').getNestedArray('antennas'), [17, 34]);
    assert.deepEqual(diced.drillUp('location', 'continent').getNestedArray('antennas'), [[16, 32], [1, 2]]);
    assert.deepEqual(diced.getNestedArray('antennas'), [[16, 32], [1, 2]]);
    // duplicates: only the last occurrence of an item receives the cells (reference Map semantics)
    const dup = cube.storedMeasures.antennas.dice(cube.dimensions, [new GenericDimension('location', 'city', ['paris', 'tokyo', 'paris']), cube.dimensions[1]]);
    assert.deepEqual(dup.data, [0, 0, 16, 32, 1, 2]);
  });
  it('a slice stays pending and the whole slice -> dice -> drillUp chain is one selection over the source', () => {
    const cube = testCube();
    const winter = cube.slice('period', 'season', 'winter'); // dice to one item + roll-up of that single item
    assert.ok(winter.storedMeasures.antennas._pending, 'the single-member roll-up moved no cells');
    const chain = winter.dice('location', 'city', ['tokyo', 'paris']).drillUp('location', 'all');
    assert.deepEqual(chain.getNestedArray('antennas'), [34]);
    assert.deepEqual(winter.getNestedArray('antennas'), [2, 8, 32]);
    assert.deepEqual(cube.slice('location', 'city', 'toledo').slice('period', 'season', 'summer').getNestedArray('routers'), 4);
  });
  it('a diced cube is independent of later writes to its source (copy-on-write of the lent buffer)', () => {
    const cube = testCube();
    const diced = cube.dice('location', 'city', ['paris', 'tokyo']);
    const sliced = cube.slice('period', 'season', 'summer');
    cube.setNestedArray('antennas', [[100, 200], [300, 400], [500, 600]]);
    cube.storedMeasures.routers.setValue(0, 77);
    assert.deepEqual(diced.getNestedArray('antennas'), [[1, 2], [16, 32]]);
    assert.deepEqual(diced.getNestedArray('routers'), [[3, 2], [16, 32]]);
    assert.deepEqual(sliced.getNestedArray('antennas'), [1, 4, 16]);
    assert.deepEqual(cube.getNestedArray('antennas'), [[100, 200], [300, 400], [500, 600]]);
    assert.deepEqual(cube.dice('location', 'city', ['toledo']).getNestedArray('antennas'), [[300, 400]]);
    cube.fillData('antennas', 9);
    assert.deepEqual(cube.getNestedArray('antennas'), [[9, 9], [9, 9], [9, 9]]);
  });
});

describe('pending selections against eager execution (seeded random chains)', () => {
  // the same chain of slice / dice / drillUp / removeDimension run lazily (selections stay pending
  // and fuse) and eagerly (cells read back after every step, which materialises each store)
  let state = 20240807;
  const rand = (n) => {
    state = (Math.imul(state, 1664525) + 1013904223) | 0;
    return (state >>> 8) % n;
  };
  const build = () => {
    const sizes = [5, 4, 3, 6];
    const dims = sizes.map((n, d) => {
      const dim = new GenericDimension(`d${d}`, 'item', Array.from({ length: n }, (_x, i) => `d${d}i${i}`));
      dim.addAttribute('item', 'parity', (item) => (Number(item.slice(-1)) % 2 ? 'odd' : 'even'));
      return dim;
    });
    const cube = new Cube(dims);
    cube.createStoredMeasure('sum_m', {}, 'float32', 0);
    cube.createStoredMeasure('last_m', Object.fromEntries(dims.map((d) => [d.id, 'last'])), 'int32', NaN_);
    const n = sizes.reduce((a, b) => a * b, 1);
    cube.setData('sum_m', Array.from({ length: n }, (_x, i) => ((i * 7) % 11 === 0 ? 0 : (i % 13) + 0.5)));
    cube.setData('last_m', Array.from({ length: n }, (_x, i) => ((i * 5) % 7 === 0 ? NaN_ : i % 17)));
    return cube;
  };
  const step = (cube, eager) => {
    if (cube.dimensions.length === 0) return cube;
    const dim = cube.dimensions[rand(cube.dimensions.length)];
    const items = dim.getItems();
    let next;
    switch (rand(5)) {
      case 0:
        next = cube.slice(dim.id, dim.rootAttribute, items[rand(items.length)]);
        break;
      case 1: {
        const keep = items.filter(() => rand(3) > 0);
        next = cube.dice(dim.id, dim.rootAttribute, keep.length ? keep : [items[0]], rand(2) === 1);
        break;
      }
      case 2:
        next = dim.attributes.includes('parity') && dim.rootAttribute !== 'parity' ? cube.drillUp(dim.id, 'parity') : cube.drillUp(dim.id, 'all');
        break;
      case 3:
        next = cube.removeDimension(dim.id);
        break;
      default:
        next = dim.attributes.includes('parity') ? cube.dice(dim.id, 'parity', [rand(2) ? 'odd' : 'even']) : cube;
    }
    if (eager) for (const id of next.storedMeasureIds) next.getData(id);
    return next;
  };
  it('120 chains of up to 5 operations agree cell for cell', () => {
    for (let chain = 0; chain < 120; ++chain) {
      const seed = state;
      const length = 1 + rand(5);
      const run = (eager) => {
        state = seed;
        rand(5);
        let cube = build();
        for (let i = 0; i < length; ++i) cube = step(cube, eager);
        return cube;
      };
      const lazy = run(false);
      const after = state;
      const eager = run(true);
      state = after;
      assert.deepEqual(lazy.dimensionIds, eager.dimensionIds, `chain ${chain}`);
      for (const id of ['sum_m', 'last_m']) {
        assert.deepEqual(lazy.getNestedArray(id), eager.getNestedArray(id), `chain ${chain} ${id}`);
        assert.deepEqual(Array.from(lazy.getStatusMap(id).keys()), Array.from(eager.getStatusMap(id).keys()), `chain ${chain} ${id} keys`);
      }
    }
  });
});

describe('collapse', () => {
  const chain = (cube) => cube.dimensionIds.reduce((c, id) => c.slice(id, 'all', 'all'), cube);
  it('additive rules: one total per measure equals the chain of slices', () => {
    const cube = testCube();
    cube.createStoredMeasure('signal', {}, 'float32', NaN_);
    cube.setNestedArray('signal', [[0.5, NaN_], [NaN_, 2.25], [4, NaN_]]);
    cube.createStoredMeasure('empty_nan', {}, 'int32', NaN_);
    cube.createStoredMeasure('empty_zero', {}, 'float32', 0);
    cube.createComputedMeasure('ratio', 'routers / antennas');
    const fast = cube.collapse();
    const slow = chain(cube);
    assert.deepEqual(fast.dimensionIds, []);
    for (const id of cube.storedMeasureIds) {
      assert.deepEqual(fast.getData(id), slow.getData(id), id);
      assert.deepEqual(Array.from(fast.getStatusMap(id).keys()), Array.from(slow.getStatusMap(id).keys()), `${id} keys`);
    }
    assert.deepEqual(fast.getData('antennas'), [63]);
    assert.deepEqual(fast.getData('signal'), [6.75]);
    assert.deepEqual(fast.storedMeasuresRules, slow.storedMeasuresRules);
    assert.deepEqual(fast.getData('ratio'), slow.getData('ratio'));
    assert.deepEqual(fast.getData('ratio'), [66 / 63]);
  });
  it('any other rule keeps the chain (an average of averages is not the overall average)', () => {
    const cube = new Cube([new GenericDimension('a', 'item', ['x', 'y']), new GenericDimension('b', 'item', ['p', 'q', 'r'])]);
    cube.createStoredMeasure('avg_m', { a: 'average', b: 'sum' }, 'float32', 0);
    cube.setNestedArray('avg_m', [[1, 2, 3], [4, 0, 6]]);
    assert.deepEqual(cube.collapse().getData('avg_m'), chain(cube).getData('avg_m'));
    assert.deepEqual(cube.collapse().getData('avg_m'), [(1 + 4) / 2 + 2 / 1 + (3 + 6) / 2]);
  });
});

describe('dimensions', () => {
  it('removeDimension with every aggregator', () => {
    let cube = new Cube([new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']), new GenericDimension('period', 'season', ['summer', 'winter'])]);
    for (const agg of ['sum', 'average', 'highest', 'lowest', 'first', 'last', 'product']) {
      cube.createStoredMeasure(`antennas_${agg}`, { period: agg, location: agg }, 'float32', 0);
      cube.setNestedArray(`antennas_${agg}`, [[1, 2], [4, 8], [16, 32]]);
    }
    cube = cube.removeDimension('location');
    assert.deepEqual(cube.getNestedArray('antennas_sum'), [21, 42]);
    assert.deepEqual(cube.getNestedArray('antennas_average'), [21 / 3, 42 / 3]);
    assert.deepEqual(cube.getNestedArray('antennas_highest'), [16, 32]);
    assert.deepEqual(cube.getNestedArray('antennas_lowest'), [1, 2]);
    assert.deepEqual(cube.getNestedArray('antennas_first'), [1, 2]);
    assert.deepEqual(cube.getNestedArray('antennas_last'), [16, 32]);
    assert.deepEqual(cube.getNestedArray('antennas_product'), [64, 512]);
  });
  it('removeDimension on empty and partially filled cubes', () => {
    const make = () => {
      const c = new Cube([new GenericDimension('location', 'root', ['paris', 'madrid', 'berlin']), new TimeDimension('time', 'month', '2010-01', '2010-02')]);
      c.createStoredMeasure('measure1', {}, 'float32', 0);
      return c;
    };
    assert.deepEqual(make().removeDimension('location').getNestedObject('measure1'), { '2010-01': 0, '2010-02': 0 });
    const c = make();
    c.hydrateFromSparseNestedObject('measure1', { paris: { '2010-01': 10, '2010-02': 0 }, madrid: { '2010-01': 0, '2010-02': 5 }, berlin: { '2010-01': 0, '2010-02': 10 } });
    assert.deepEqual(c.removeDimension('location').getNestedObject('measure1'), { '2010-01': 10, '2010-02': 15 });
  });
  it('addDimension then removeDimension round trips (generic and time)', () => {
    for (const added of [new GenericDimension('location', 'city', ['paris', 'madrid', 'berlin']), new TimeDimension('time2', 'week_mon', '2010-W01-mon', '2010-W08-mon')]) {
      const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-02')]);
      cube.createStoredMeasure('measure1', { time: 'sum' }, 'float32', 0);
      cube.createStoredMeasure('measure2', { time: 'average' }, 'float32', 0);
      cube.hydrateFromSparseNestedObject('measure1', { '2010-01': 100, '2010-02': 100 });
      cube.hydrateFromSparseNestedObject('measure2', { '2010-01': 100, '2010-02': 100 });
      const bigger = cube.addDimension(added, { measure1: 'sum', measure2: 'average' });
      assert.equal(bigger.storeSize, 2 * added.numItems);
      const back1 = bigger.removeDimension(added.id).getNestedObject('measure1');
      // float32 storage: 100/3 is rounded per cell; the reference keeps float64 (1e-5 relative)
      for (const k of Object.keys(back1)) assert.ok(Math.abs(back1[k] - 100) <= 1e-5 * 100, `measure1 ${k} ${back1[k]}`);
      assert.deepEqual(bigger.removeDimension(added.id).getNestedObject('measure2'), cube.getNestedObject('measure2'));
    }
  });
  it('reorderDimensions', () => {
    assert.deepEqual(testCube().reorderDimensions(['period', 'location']).getNestedArray('antennas'), [[1, 4, 16], [2, 8, 32]]);
    const cube = new Cube([new GenericDimension('dim1', 'item', ['11', '12']), new GenericDimension('dim2', 'item', ['21', '22']), new GenericDimension('dim3', 'item', ['31', '32'])]);
    cube.createStoredMeasure('main');
    cube.setData('main', [1, 2, 3, 4, 5, 6, 7, 8]);
    assert.equal(cube.reorderDimensions(['dim1', 'dim2', 'dim3']), cube);
    assert.deepEqual(cube.reorderDimensions(['dim1', 'dim3', 'dim2']).getNestedObject('main'), { 11: { 31: { 21: 1, 22: 3 }, 32: { 21: 2, 22: 4 } }, 12: { 31: { 21: 5, 22: 7 }, 32: { 21: 6, 22: 8 } } });
    assert.deepEqual(cube.reorderDimensions(['dim3', 'dim2', 'dim1']).getNestedObject('main'), { 31: { 21: { 11: 1, 12: 5 }, 22: { 11: 3, 12: 7 } }, 32: { 21: { 11: 2, 12: 6 }, 22: { 11: 4, 12: 8 } } });
    assert.deepEqual(cube.reorderDimensions(['dim3', 'dim1', 'dim2']).getNestedObject('main'), { 31: { 11: { 21: 1, 22: 3 }, 12: { 21: 5, 22: 7 } }, 32: { 11: { 21: 2, 22: 4 }, 12: { 21: 6, 22: 8 } } });
  });
});

describe('hydrateFromCube', () => {
  const big = () => {
    const c = new Cube([new GenericDimension('period', 'season', ['summer', 'winter']), new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo'])]);
    c.createStoredMeasure('antennas', {}, 'uint32', 0);
    return c;
  };
  const zeros = { summer: { paris: 0, toledo: 0, tokyo: 0 } };
  it('missing / extra measures, missing data', () => {
    const cube = big();
    const small = new Cube([new GenericDimension('period', 'season', ['winter']), new GenericDimension('location', 'city', ['paris', 'tokyo'])]);
    small.createStoredMeasure('otherMeasure', {}, 'uint32', NaN_);
    cube.hydrateFromCube(small);
    assert.deepEqual(cube.getNestedObject('antennas'), Object.assign({}, zeros, { winter: { paris: 0, toledo: 0, tokyo: 0 } }));
    small.createStoredMeasure('antennas', {}, 'uint32');
    small.setNestedObject('antennas', { winter: { paris: 10, tokyo: 20 } });
    cube.hydrateFromCube(small);
    assert.deepEqual(cube.getNestedObject('antennas'), Object.assign({}, zeros, { winter: { paris: 10, toledo: 0, tokyo: 20 } }));
  });
  it('extra item in the small cube, item order differs', () => {
    const cube = big();
    const small = new Cube([new GenericDimension('period', 'season', ['winter']), new GenericDimension('location', 'city', ['tokyo', 'losangeles', 'paris'])]);
    small.createStoredMeasure('antennas', {}, 'uint32', 0);
    small.setNestedObject('antennas', { winter: { tokyo: 1, losangeles: 2, paris: 3 } });
    cube.hydrateFromCube(small);
    assert.deepEqual(cube.getNestedObject('antennas'), Object.assign({}, zeros, { winter: { paris: 3, toledo: 0, tokyo: 1 } }));
  });
  it('extra dimension in the small cube is summed away', () => {
    const cube = big();
    const small = new Cube([new GenericDimension('period', 'season', ['winter']), new GenericDimension('something', 'root', ['a', 'b', 'c']), new GenericDimension('location', 'city', ['paris', 'tokyo'])]);
    small.createStoredMeasure('antennas', {}, 'uint32', 0);
    small.setNestedObject('antennas', { winter: { a: { paris: 1, tokyo: 2 }, b: { paris: 3, tokyo: 4 }, c: { paris: 5, tokyo: 6 } } });
    cube.hydrateFromCube(small);
    assert.deepEqual(cube.getNestedObject('antennas'), Object.assign({}, zeros, { winter: { paris: 9, toledo: 0, tokyo: 12 } }));
  });
  it('missing dimension is spread with integer remainders (32 -> 11,10,11)', () => {
    const cube = big();
    const small = new Cube([new GenericDimension('period', 'season', ['winter'])]);
    small.createStoredMeasure('antennas', {}, 'uint32', 0);
    small.setNestedObject('antennas', { winter: 32 });
    cube.hydrateFromCube(small);
    assert.deepEqual(cube.getNestedObject('antennas'), Object.assign({}, zeros, { winter: { paris: 11, toledo: 10, tokyo: 11 } }));
  });
  it('drillUp and drillDown on the way (months <-> quarters)', () => {
    const q = new Cube([new TimeDimension('time', 'quarter', '2010-Q1', '2010-Q3'), new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo'])]);
    q.createStoredMeasure('antennas', {}, 'uint32', 0);
    const m = new Cube([new TimeDimension('time', 'month', '2010-04', '2010-06'), new GenericDimension('location', 'city', ['toledo'])]);
    m.createStoredMeasure('antennas', {}, 'uint32', 0);
    m.setNestedObject('antennas', { '2010-04': { toledo: 1 }, '2010-05': { toledo: 2 }, '2010-06': { toledo: 3 } });
    q.hydrateFromCube(m);
    assert.deepEqual(q.getNestedObject('antennas'), { '2010-Q1': { paris: 0, toledo: 0, tokyo: 0 }, '2010-Q2': { paris: 0, toledo: 6, tokyo: 0 }, '2010-Q3': { paris: 0, toledo: 0, tokyo: 0 } });

    const months = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-06'), new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo'])]);
    months.createStoredMeasure('antennas', {}, 'uint32', 0);
    const quarter = new Cube([new TimeDimension('time', 'quarter', '2010-Q2', '2010-Q2'), new GenericDimension('location', 'city', ['toledo'])]);
    quarter.createStoredMeasure('antennas', {}, 'uint32', 0);
    quarter.setNestedObject('antennas', { '2010-Q2': { toledo: 100 } });
    months.hydrateFromCube(quarter);
    const z = { paris: 0, toledo: 0, tokyo: 0 };
    assert.deepEqual(months.getNestedObject('antennas'), { '2010-01': z, '2010-02': z, '2010-03': z, '2010-04': { paris: 0, toledo: 34, tokyo: 0 }, '2010-05': { paris: 0, toledo: 33, tokyo: 0 }, '2010-06': { paris: 0, toledo: 33, tokyo: 0 } });
  });
});

describe('compose (test/cube-to-cube.js:5-401, stored-measure cases)', () => {
  const period = () => new GenericDimension('period', 'season', ['summer', 'winter']);
  const cities = (items) => new GenericDimension('location', 'city', items);
  const grid = [[1, 2], [4, 8], [16, 32]];
  function pair(dims1, data1, dims2, data2, def) {
    const c1 = new Cube(dims1);
    const c2 = new Cube(dims2);
    if (def === undefined) {
      c1.createStoredMeasure('antennas');
      c2.createStoredMeasure('routers');
    } else {
      c1.createStoredMeasure('antennas', {}, 'float32', def);
      c2.createStoredMeasure('routers', {}, 'float32', def);
    }
    c1.setNestedArray('antennas', data1);
    c2.setNestedArray('routers', data2);
    return [c1, c2];
  }
  for (const union of [false, true]) {
    const tag = union ? 'union' : 'intersection';
    // union() sorts the merged items, so the union cases start from the sorted order as the reference's do
    const order = union ? ['paris', 'tokyo', 'toledo'] : ['paris', 'toledo', 'tokyo'];
    it(`${tag}: same dimensions`, () => {
      const loc = cities(order);
      const per = period();
      const [c1, c2] = pair([loc, per], grid, [loc, per], [[3, 2], [4, 9], [16, 32]]);
      const c = c1.compose(c2, union);
      assert.deepEqual(c.dimensionIds, ['location', 'period']);
      assert.deepEqual(c.getNestedArray('routers'), [[3, 2], [4, 9], [16, 32]]);
      assert.deepEqual(c.getNestedArray('antennas'), grid);
    });
    it(`${tag}: a dimension missing from one cube is summed away`, () => {
      const loc = cities(order);
      const [c1, c2] = pair([loc, period()], grid, [loc], [3, 4, 16]);
      const c = c1.compose(c2, union);
      assert.deepEqual(c.dimensionIds, ['location']);
      assert.deepEqual(c.getNestedArray('antennas'), [3, 12, 48]);
      assert.deepEqual(c.getNestedArray('routers'), [3, 4, 16]);
    });
    it(`${tag}: same time dimension`, () => {
      const time = new TimeDimension('time', 'month', '2010-01', '2010-02');
      const [c1, c2] = pair([time], [1, 2], [time], [3, 2]);
      const c = c1.compose(c2, union);
      assert.deepEqual(c.dimensionIds, ['time']);
      assert.deepEqual(c.getNestedArray('antennas'), [1, 2]);
      assert.deepEqual(c.getNestedArray('routers'), [3, 2]);
    });
  }
  it('intersection: items missing from both cubes', () => {
    const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]]);
    const c = c1.compose(c2);
    assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [16, 32]]);
    assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [256, 512]]);
  });
  it('union: items missing from both cubes (NaN default)', () => {
    const [c1, c2] = pair([cities(['paris', 'toledo', 'tokyo']), period()], grid, [cities(['soria', 'tokyo', 'paris']), period()], [[64, 128], [256, 512], [1024, 2048]], NaN_);
    const c = c1.compose(c2, true);
    assert.deepEqual(c.getDimension('location').getItems(), ['paris', 'soria', 'tokyo', 'toledo']);
    assert.deepEqual(c.getNestedArray('antennas'), [[1, 2], [NaN_, NaN_], [16, 32], [4, 8]]);
    assert.deepEqual(c.getNestedArray('routers'), [[1024, 2048], [64, 128], [256, 512], [NaN_, NaN_]]);
  });
  it('overlapping time dimensions', () => {
    const t = (a, b, root = 'month') => new TimeDimension('time', root, a, b);
    let [c1, c2] = pair([t('2010-01', '2010-02')], [1, 2], [t('2010-02', '2010-03')], [3, 2], NaN_);
    assert.deepEqual(c1.compose(c2).getNestedArray('antennas'), [2]);
    assert.deepEqual(c1.compose(c2).getNestedArray('routers'), [3]);
    assert.deepEqual(c1.compose(c2, true).getData('antennas'), [1, 2, NaN_]);
    assert.deepEqual(c1.compose(c2, true).getData('routers'), [NaN_, 3, 2]);
    [c1, c2] = pair([t('2010-01', '2010-02')], [1, 2], [t('2010-03', '2010-04')], [3, 2], NaN_);
    assert.equal(c1.compose(c2).storeSize, 0);
    assert.deepEqual(c1.compose(c2, true).getData('antennas'), [1, 2, NaN_, NaN_]);
    assert.deepEqual(c1.compose(c2, true).getData('routers'), [NaN_, NaN_, 3, 2]);
    [c1, c2] = pair([t('2010-01', '2010-04')], [1, 2, 4, 8], [t('2010-Q1', '2010-Q3', 'quarter')], [16, 32, 64]);
    assert.deepEqual(c1.compose(c2).getNestedArray('antennas'), [7, 8]);
    assert.deepEqual(c1.compose(c2).getNestedArray('routers'), [16, 32]);
    [c1, c2] = pair([t('2010-01', '2010-04')], [1, 2, 4, 8], [t('2010-Q1', '2010-Q3', 'quarter')], [16, 32, 64], NaN_);
    assert.deepEqual(c1.compose(c2, true).getData('antennas'), [7, 8, NaN_]);
    assert.deepEqual(c1.compose(c2, true).getData('routers'), [16, 32, 64]);
  });
});

describe('computed measures (formula.js + the device interpreter)', () => {
  const withComputed = () => {
    const cube = testCube();
    cube.createComputedMeasure('router_by_antennas', 'routers / antennas');
    return cube;
  };
  it('evaluates the reference fixture formula per cell', () => {
    const cube = withComputed();
    assert.deepEqual(cube.getData('router_by_antennas'), [3 / 1, 2 / 2, 4 / 4, 9 / 8, 16 / 16, 32 / 32]);
    assert.equal(cube.getSingleData('router_by_antennas', { location: 'toledo', period: 'winter' }), 9 / 8);
    assert.deepEqual(cube.computedMeasureIds, ['router_by_antennas']);
    // derived cubes carry the formula and evaluate it on their own (aggregated) cells
    assert.deepEqual(cube.drillUp('location', 'continent').getNestedArray('router_by_antennas'), [[7 / 5, 11 / 10], [1, 1]]);
    assert.deepEqual(cube.slice('period', 'season', 'winter').getData('router_by_antennas'), [1, 9 / 8, 1]);
  });
  it('totals, inlining of other computed measures, unknown measures', () => {
    const cube = withComputed();
    cube.createComputedMeasure('share', 'antennas / antennas__total');
    assert.deepEqual(cube.getData('share'), [1, 2, 4, 8, 16, 32].map((v) => v / 63));
    cube.createComputedMeasure('twice', 'router_by_antennas * 2');
    assert.deepEqual(cube.getData('twice'), [6, 2, 2, 9 / 4, 2, 2]);
    assert.throws(() => cube.createComputedMeasure('bad', 'antennas + nothing'), /Unknown measure\(s\): nothing/);
    assert.throws(() => cube.createComputedMeasure('antennas', 'routers'), /This measure already exists antennas/);
  });
  it('NaN-coalescing || (test/cube-to-cube.js:355-382)', () => {
    const t = (a, b) => new TimeDimension('time', 'month', a, b);
    const c1 = new Cube([t('2010-01', '2010-02')]);
    c1.createStoredMeasure('antennas', {}, 'float32', NaN_);
    c1.setNestedArray('antennas', [1, 2]);
    const c2 = new Cube([t('2010-03', '2010-04')]);
    c2.createStoredMeasure('routers', {}, 'float32', NaN_);
    c2.setNestedArray('routers', [3, 2]);
    const c = c1.compose(c2, true);
    c.createComputedMeasure('safe_sum', 'antennas + routers');
    c.createComputedMeasure('unsafe_sum', 'antennas || routers');
    assert.deepEqual(c.getData('safe_sum'), [NaN_, NaN_, NaN_, NaN_]);
    assert.deepEqual(c.getData('unsafe_sum'), [1, 2, 3, 2]);
  });
  it('rename / drop keep formulas consistent (test/cube-rename.js)', () => {
    const cube = withComputed();
    assert.throws(() => cube.renameMeasure('missing', 'missing2'));
    const a = cube.clone();
    a.renameMeasure('router_by_antennas', 'router_by_receivers');
    assert.doesNotThrow(() => a.getData('router_by_receivers'));
    assert.throws(() => a.getData('router_by_antennas'));
    const b = cube.clone();
    b.renameMeasure('antennas', 'receivers');
    assert.deepEqual(b.getData('router_by_antennas'), cube.getData('router_by_antennas'));
    assert.throws(() => b.getData('antennas'));
    b.dropMeasure('receivers');
    assert.deepEqual(b.computedMeasureIds, []);
    const c = cube.clone();
    c.convertToStoredMeasure('router_by_antennas', {}, 'float32', 0);
    assert.deepEqual(c.storedMeasureIds, ['antennas', 'routers', 'router_by_antennas']);
    assert.deepEqual(c.getData('router_by_antennas'), [3, 1, 1, 1.125, 1, 1]);
  });
  it('device interpreter agrees with the host evaluator AND with plain JavaScript closures on every operator and function', () => {
    const n = 4096;
    const cube = new Cube([new GenericDimension('d', 'root', Array.from({ length: n }, (_x, i) => `i${i}`))]);
    cube.createStoredMeasure('aa', {}, 'float64', NaN_);
    cube.createStoredMeasure('bb', {}, 'float32', 0);
    cube.createStoredMeasure('cc', {}, 'int32', NaN_);
    let seed = 12345;
    const rnd = () => ((seed = (Math.imul(seed, 1664525) + 1013904223) | 0) >>> 0) / 4294967296;
    cube.setData('aa', Array.from({ length: n }, () => (rnd() < 0.2 ? NaN_ : (rnd() - 0.5) * 20)));
    cube.setData('bb', Array.from({ length: n }, () => (rnd() < 0.3 ? 0 : Math.fround(rnd() * 8))));
    cube.setData('cc', Array.from({ length: n }, () => (rnd() < 0.3 ? NaN_ : Math.floor(rnd() * 21) - 10)));
    const formulas = ['aa + bb * cc - 2', 'aa / bb', 'cc % 3 + 2 ^ bb', '-aa || bb', 'abs aa + sqrt(bb) + floor(aa / 3) + ceil aa + round(aa) + trunc aa',
      'min(aa, bb, cc) + max(aa, 1) * hypot(bb, cc)', 'bb ? aa : cc', 'if(isNaN(aa), bb, aa) + not bb', 'exp(bb / 4) + ln(bb + 1) + log10(bb + 1) + log2(bb + 2) + cbrt aa',
      'sin aa + cos(aa) * tan(bb / 10) + atan2(aa, bb) + asin(bb / 8) + acos(bb / 8) + atan cc', 'sign(aa) * roundTo(aa, 2) + PI * E', 'aa__total + bb__total / cc__total', '(aa + 1) * (bb - 2) / (cc + 0.5) ^ 2',
      '1 ^ aa', 'round(aa / 7)'];
    // An INDEPENDENT restatement of the same formulas as plain JavaScript closures (neither formula.js's parser nor its
    // evaluator is involved): expr-eval's published operator semantics (^ = Math.pow, % = JS remainder, ?: and if() by
    // truthiness, `not`, roundTo(x, n) = round at n decimals), with `||` and isNaN exactly as the reference
    // redefines them in src/parser.js:11-23.
    const nanAdd = (a, b) => (Number.isNaN(a) && !Number.isNaN(b) ? b : !Number.isNaN(a) && Number.isNaN(b) ? a : a + b);
    const roundTo = (x, d) => +(`${Math.round(`${x}e+${d}`)}e-${d}`);
    const plain = [
      (a, b, c) => a + b * c - 2, (a, b) => a / b, (a, b, c) => (c % 3) + Math.pow(2, b), (a, b) => nanAdd(-a, b),
      (a, b) => Math.abs(a) + Math.sqrt(b) + Math.floor(a / 3) + Math.ceil(a) + Math.round(a) + Math.trunc(a),
      (a, b, c) => Math.min(a, b, c) + Math.max(a, 1) * Math.hypot(b, c), (a, b, c) => (b ? a : c), (a, b) => (Number.isNaN(a) ? b : a) + !b,
      (a, b) => Math.exp(b / 4) + Math.log(b + 1) + Math.log10(b + 1) + Math.log2(b + 2) + Math.cbrt(a),
      (a, b, c) => Math.sin(a) + Math.cos(a) * Math.tan(b / 10) + Math.atan2(a, b) + Math.asin(b / 8) + Math.acos(b / 8) + Math.atan(c),
      (a) => Math.sign(a) * roundTo(a, 2) + Math.PI * Math.E, (a, b, c, t) => t.aa__total + t.bb__total / t.cc__total,
      (a, b, c) => ((a + 1) * (b - 2)) / Math.pow(c + 0.5, 2), (a) => Math.pow(1, a), (a) => Math.round(a / 7)];
    const close = (x, y) => (Number.isNaN(x) && Number.isNaN(y)) || x === y || Math.abs(x - y) <= 1e-12 * Math.max(1, Math.abs(x));
    formulas.forEach((formula, k) => {
      cube.createComputedMeasure(`f_${k}x`, formula);
      const device = cube.getData(`f_${k}x`);
      const expression = cube.computedMeasures[`f_${k}x`];
      const [A, B, C] = ['aa', 'bb', 'cc'].map((m) => cube.getData(m));
      const totals = { aa__total: cube.getTotal('aa'), bb__total: cube.getTotal('bb'), cc__total: cube.getTotal('cc') };
      for (let i = 0; i < n; ++i) {
        const host = expression.evaluate(Object.assign({ aa: A[i], bb: B[i], cc: C[i] }, totals));
        assert.ok(close(host, device[i]), `${formula} @${i}: host ${host} device ${device[i]} (aa=${A[i]} bb=${B[i]} cc=${C[i]})`);
        const independent = plain[k](A[i], B[i], C[i], totals);
        assert.ok(close(independent, device[i]), `${formula} @${i}: plain JavaScript ${independent} device ${device[i]} (aa=${A[i]} bb=${B[i]} cc=${C[i]})`);
      }
    });
  });
  it('formulas survive serialisation', () => {
    const cube = withComputed();
    const copy = Cube.deserialize(cube.serialize());
    assert.deepEqual(copy.computedMeasureIds, ['router_by_antennas']);
    assert.deepEqual(copy.getData('router_by_antennas'), cube.getData('router_by_antennas'));
  });
});

describe('serialisation (test/cube-serialize.js + blobs written by the reference)', () => {
  const { HipStore, wire } = require('../../olap-in-memory_amd/js');
  const golden = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'wire.json'), 'utf8')).cases;
  const bytes = (b64) => wire.toArrayBuffer(Buffer.from(b64, 'base64'));
  it('reads store blobs written by the reference and writes the same bytes back', () => {
    for (const key of ['store', 'storeNanDefault']) {
      const g = golden[key];
      const store = HipStore.deserialize(bytes(g.blob));
      assert.equal(store.size, g.dump.size);
      assert.equal(store._type, g.type);
      assert.deepEqual(Array.from(store._dataMap.keys()), g.dump.keys);
      assert.deepEqual(Array.from(store._dataMap.values()), g.dump.values.map((v) => (g.type === 'float32' ? Math.fround(Number(v)) : Number(v))));
      const mine = store.serialize();
      assert.deepEqual(wire.fromBuffer(mine), wire.fromBuffer(bytes(g.blob)));
      // byte-identical too, except that a NaN default's payload bits are whatever V8 held (not observable in JS)
      if (key === 'store') assert.equal(Buffer.from(mine).toString('base64'), g.blob, `${key}: byte-identical blob`);
      else assert.equal(mine.byteLength, bytes(g.blob).byteLength);
    }
  });
  it('cube round trip, 50 x 50 x 13 cells', () => {
    const items = [];
    for (let i = 0; i < 50; ++i) items.push(i.toString());
    const cube = new Cube([new GenericDimension('dim1', 'root', items), new GenericDimension('dim2', 'root', items), new TimeDimension('time', 'month', '2010-01', '2011-01')]);
    cube.createStoredMeasure('main', { time: 'average' }, 'float32', 0);
    cube.setData('main', Array.from({ length: 50 * 50 * 13 }).map((_v, i) => (i % 7 === 0 ? 0 : 30 + (i % 5))));
    const copy = Cube.deserialize(cube.serialize());
    assert.deepEqual(copy.getNestedObject('main'), cube.getNestedObject('main'));
    assert.deepEqual(copy.storedMeasuresRules, cube.storedMeasuresRules);
    assert.deepEqual(Cube.deserializeFromBase64String(cube.serializeToBase64String()).getData('main'), cube.getData('main'));
    assert.deepEqual(copy.drillUp('time', 'year').getData('main'), cube.drillUp('time', 'year').getData('main'));
  });
});

describe('BASELINE config 1 through the Cube API', () => {
  it('[10,10,10] drillUp(dimension0, all) equals the reference output', () => {
    const golden = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'configs.json'), 'utf8')).cases.find((c) => c.name === 'config1_10x10x10_dim0');
    const dims = [0, 1, 2].map((i) => new GenericDimension(`dimension${i}`, 'root', Array.from({ length: 10 }, (_x, j) => `dimension${i}-item${j}`)));
    const cube = new Cube(dims);
    cube.createStoredMeasure('measure0', {}, 'float32', 0);
    // mulberry32, two draws per cell (value, Bernoulli mask), as oracle/gen_golden.js configCube()
    let a = golden.seed | 0;
    const rnd = () => {
      a = (a + 0x6d2b79f5) | 0;
      let t = Math.imul(a ^ (a >>> 15), 1 | a);
      t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t;
      return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
    };
    const values = [];
    for (let i = 0; i < 1000; ++i) {
      values.push(Math.fround(0.5 + rnd()));
      rnd();
    }
    cube.setData('measure0', values);
    const up = cube.drillUp('dimension0', 'all');
    assert.equal(up.storeSize, 100);
    assert.deepEqual(up.getData('measure0'), golden.out.map((v) => Math.fround(Number(v))));
    assert.deepEqual(cube.slice('dimension0', 'all', 'all').getData('measure0'), up.getData('measure0'));
  });
});

describe('insertion order (measures with a first / last rule keep the reference Map order)', () => {
  const make = (rules) => {
    const cube = new Cube([new GenericDimension('period', 'season', ['summer', 'winter']), new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo'])]);
    cube.createStoredMeasure('mm', rules, 'float32', 0);
    // object key order = insertion order (src/cube.js:479): cells 5, 3, 1
    cube.hydrateFromSparseNestedObject('mm', { winter: { tokyo: 5, paris: 6 }, summer: { toledo: 7 } });
    return cube;
  };
  it('keys(), first-hit order of a roll-up, last by insertion order', () => {
    const cube = make({ period: 'first', location: 'last' });
    assert.equal(cube.storedMeasures.mm.orderTracked, 2);
    assert.deepEqual(Array.from(cube.getStatusMap('mm').keys()), [5, 3, 1]);
    const byCity = cube.drillUp('period', 'all');
    assert.deepEqual(byCity.getData('mm'), [6, 7, 5]);
    assert.deepEqual(Array.from(byCity.getStatusMap('mm').keys()), [2, 0, 1]); // tokyo was visited first, then paris, then toledo
    assert.deepEqual(byCity.drillUp('location', 'all').getData('mm'), [7]); // the LAST inserted: toledo (by index it would be tokyo's 5)
    assert.deepEqual(cube.collapse().getData('mm'), [7]);
    assert.deepEqual(cube.getNestedObject('mm', true).all, { paris: 6, toledo: 7, tokyo: 5, all: 7 });
    const back = Cube.deserialize(cube.serialize());
    assert.deepEqual(Array.from(back.getStatusMap('mm').keys()), [5, 3, 1]);
    assert.deepEqual(back.drillUp('period', 'all').drillUp('location', 'all').getData('mm'), [7]);
  });
  it('a measure without such a rule is not tracked and answers by flat index', () => {
    const cube = make({ period: 'sum', location: 'sum' });
    assert.equal(cube.storedMeasures.mm.orderTracked, 0);
    assert.deepEqual(Array.from(cube.getStatusMap('mm').keys()), [1, 3, 5]);
  });
});

describe('measures that share a rule are rolled up in one launch (HipStore.drillUpMany)', () => {
  it('equals the per-measure roll-ups: mixed cell types, defaults and rules, a lazily diced measure', () => {
    const items = (name, n) => Array.from({ length: n }, (_, i) => `${name}${i}`);
    const a = new GenericDimension('da', 'item', items('a', 7));
    a.addAttribute('item', 'pair', Object.fromEntries(items('a', 7).map((it, i) => [it, `p${i % 3}`])));
    const dims = [a, new GenericDimension('db', 'item', items('b', 6)), new GenericDimension('dc', 'item', items('c', 5))];
    const cube = new Cube(dims);
    const specs = [['s1', 'sum', 'float32', 0], ['s2', 'sum', 'float32', 0], ['s3', 'sum', 'float32', 0], ['av', 'average', 'float32', 0],
      ['i1', 'sum', 'int32', 0], ['i2', 'sum', 'int32', 0], ['n1', 'sum', 'float32', NaN_], ['n2', 'sum', 'float32', NaN_], ['u1', 'highest', 'uint32', NaN_], ['u2', 'highest', 'uint32', NaN_]];
    let seed = 12345;
    const rnd = () => ((seed = (seed * 1103515245 + 12345) % 2147483648) / 2147483648);
    for (const [id, rule, type, def] of specs) {
      cube.createStoredMeasure(id, { da: rule, db: rule, dc: rule }, type, def);
      cube.setData(id, Array.from({ length: 210 }, () => (rnd() < 0.3 ? def : Math.floor(rnd() * 17) - (type === 'uint32' ? 0 : 8))));
    }
    for (const [dim, attr] of [['da', 'pair'], ['da', 'all'], ['db', 'all'], ['dc', 'all']]) {
      const together = cube.drillUp(dim, attr);
      for (const [id, rule] of specs) {
        const index = cube.getDimensionIndex(dim);
        const alone = cube.storedMeasures[id].drillUp(cube.dimensions, together.dimensions, rule);
        assert.deepEqual(together.getData(id), alone.data, `${id} ${dim}->${attr}`);
        assert.deepEqual(Array.from(together.getStatusMap(id).keys()), Array.from(alone._dataMap.keys()), `${id} ${dim}->${attr} keys`);
        assert.equal(index >= 0, true);
      }
    }
    // a slice keeps its selection pending: those measures take the fused single-store path, same values
    const sliced = cube.dice('db', 'item', ['b1', 'b4']);
    const viaBatch = sliced.drillUp('da', 'pair');
    for (const [id] of specs) assert.deepEqual(viaBatch.getData(id), cube.drillUp('da', 'pair').dice('db', 'item', ['b1', 'b4']).getData(id), id);
  });
});

describe('integer measures hold the reference Map\'s float64 numbers (in-memory.js:77-92 coerces only in serialize())', () => {
  const { HipStore, wire, backend } = require('../../olap-in-memory_amd/js');
  const golden = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'store_kat.json'), 'utf8')).cases;
  const kat = (name) => golden.find((c) => c.name === name);
  const lineDims = (n, groups, id = 'd') => {
    const items = Array.from({ length: n }, (_, i) => `i${i}`);
    const dim = new GenericDimension(id, 'item', items);
    dim.addAttribute('item', 'group', Object.fromEntries(items.map((it, i) => [it, `g${groups(i)}`])));
    return dim;
  };
  it('int32 average of 7 and 8 is 7.5 (reference golden int32_average_fraction), 7 once serialized', () => {
    assert.deepEqual(kat('int32_average_fraction').out.values, [7.5]);
    const cube = new Cube([lineDims(2, () => 0)]);
    cube.createStoredMeasure('mm', { d: 'average' }, 'int32', 0);
    cube.setData('mm', [7, 8]);
    const up = cube.drillUp('d', 'all');
    assert.deepEqual(up.getData('mm'), [7.5]);
    assert.equal(up.storedMeasures.mm._type, 'int32');
    assert.equal(up.storedMeasures.mm.byteLength, 4);
    const blob = wire.fromBuffer(up.storedMeasures.mm.serialize());
    assert.ok(blob.dataBuffer instanceof Int32Array);
    assert.deepEqual(Array.from(blob.dataBuffer), [7]);
    assert.deepEqual(HipStore.deserialize(up.storedMeasures.mm.serialize()).data, [7]);
  });
  it('uint32 sum passes 2^32 without wrapping (reference golden uint32_sum_no_wrap); serialize() wraps', () => {
    assert.deepEqual(kat('uint32_sum_no_wrap').out.values, [8000000000]);
    const cube = new Cube([lineDims(2, () => 0)]);
    cube.createStoredMeasure('mm', { d: 'sum' }, 'uint32', 0);
    cube.setData('mm', [4000000000, 4000000000]);
    const up = cube.drillUp('d', 'all');
    assert.deepEqual(up.getData('mm'), [8000000000]);
    assert.deepEqual(Array.from(wire.fromBuffer(up.storedMeasures.mm.serialize()).dataBuffer), [8000000000 % 4294967296]);
  });
  it('chains keep the fractions: average of [1, 2] twice, then their sum = 3', () => {
    const cube = new Cube([lineDims(2, (i) => i, 'd0'), lineDims(2, () => 0, 'd1')]);
    cube.createStoredMeasure('mm', { d0: 'sum', d1: 'average' }, 'int32', 0);
    cube.setData('mm', [1, 2, 1, 2]);
    assert.deepEqual(cube.drillUp('d1', 'all').getData('mm'), [1.5, 1.5]);
    assert.deepEqual(cube.drillUp('d1', 'all').drillUp('d0', 'all').getData('mm'), [3]);
  });
  it('drillDown spreads the integer remainder by the DECLARED type (in-memory.js:343, :403-417) on those cells', () => {
    for (const type of ['int32', 'uint32']) {
      const cube = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-02')]);
      cube.createStoredMeasure('mm', { time: 'sum' }, type, 0);
      cube.setData('mm', [100, 7.5]);
      const days = cube.drillDown('time', 'day');
      const jan = days.getData('mm').slice(0, 31);
      assert.equal(jan.reduce((a, b) => a + b, 0), 100);
      assert.deepEqual(Array.from(new Set(jan)).sort(), [3, 4]);
      // 7.5 over 28 days, replayed with the reference's own arithmetic
      const want = [];
      for (let id = 0; id < 28; ++id) {
        const one = (7.5 % 28) / 28;
        want.push(Math.floor(Math.floor(7.5 / 28)) + (Math.floor(id * one) === Math.floor((id - 1) * one) ? 0 : 1));
      }
      assert.deepEqual(days.getData('mm').slice(31), want);
    }
    const f = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-01')]);
    f.createStoredMeasure('mm', { time: 'sum' }, 'float64', 0);
    f.setData('mm', [100]);
    assert.deepEqual(f.drillDown('time', 'day').getData('mm'), Array(31).fill(100 / 31));
  });
  it('NaN is an ordinary value of a 0-default integer measure (in-memory.js:118-133), 0 once serialized', () => {
    const store = new HipStore(3, 'int32', 0);
    store.setValue(1, Number.NaN);
    store.setValue(2, 2.25);
    assert.deepEqual(store.data, [0, Number.NaN, 2.25]);
    assert.deepEqual(Array.from(store._dataMap.keys()), [1, 2]);
    assert.deepEqual(Array.from(wire.fromBuffer(store.serialize()).dataBuffer), [0, 2]);
  });
  it('load() between an integer and a float64 measure copies the numbers as they are', () => {
    const dim = lineDims(3, () => 0);
    const a = new HipStore(3, 'int32', 0);
    a.data = [1.5, 0, -2.5];
    const b = new HipStore(3, 'float64', 0);
    b.load(a, [dim], [dim]);
    assert.deepEqual(b.data, [1.5, 0, -2.5]);
  });
  it('typed arrays narrower than the Float64 cells are widened by the addon (data = Int32Array / Uint32Array / Float32Array)', () => {
    const i32 = new HipStore(5, 'int32', 0);
    i32.data = Int32Array.of(-3, 0, 7, 2147483647, -2147483648);
    assert.deepEqual(i32.data, [-3, 0, 7, 2147483647, -2147483648]);
    assert.deepEqual(Array.from(i32._dataMap.keys()), [0, 2, 3, 4]);
    const u32 = new HipStore(3, 'uint32', Number.NaN);
    u32.data = Uint32Array.of(0, 4294967295, 5);
    assert.deepEqual(u32.data, [0, 4294967295, 5]);
    const f64 = new HipStore(3, 'float64', 0);
    f64.data = Float32Array.of(0.5, Number.NaN, 0);
    assert.deepEqual(f64.data, [0.5, Number.NaN, 0]);
    assert.deepEqual(Array.from(f64._dataMap.keys()), [0, 1]);
  });
  it('backend.setCompactIntegers(true): 4-byte typed cells, values coerced after every operation', () => {
    backend.setCompactIntegers(true);
    try {
      const cube = new Cube([lineDims(2, () => 0)]);
      cube.createStoredMeasure('mm', { d: 'average' }, 'int32', 0);
      cube.createStoredMeasure('uu', { d: 'sum' }, 'uint32', 0);
      cube.setData('mm', [7, 8]);
      cube.setData('uu', [4000000000, 4000000000]);
      assert.equal(cube.storedMeasures.mm._cells, 'int32');
      const up = cube.drillUp('d', 'all');
      assert.deepEqual(up.getData('mm'), [7]);
      assert.deepEqual(up.getData('uu'), [8000000000 % 4294967296]);
      assert.deepEqual(Array.from(wire.fromBuffer(up.storedMeasures.mm.serialize()).dataBuffer), [7]);
      const days = new Cube([new TimeDimension('time', 'month', '2010-01', '2010-01')]);
      days.createStoredMeasure('mm', { time: 'sum' }, 'uint32', 0);
      days.setData('mm', [100]);
      const jan = days.drillDown('time', 'day').getData('mm');
      assert.equal(jan.reduce((x, y) => x + y, 0), 100);
      assert.deepEqual(Array.from(new Set(jan)).sort(), [3, 4]);
    } finally {
      backend.setCompactIntegers(false);
    }
    const exact = new HipStore(2, 'int32', 0);
    assert.equal(exact._cells, 'float64');
  });
});

run();
