'use strict';
/*
 * ../../olap-in-memory_amd/js/selection.js without a GPU: the levels that Cube.getTotalForDimensionItems and
 * copyMeasureData hand to the device must enumerate the combinations of the per-cell path (src/cube.js:19-32,
 * :679-707, :859-888) in the same nesting order, and must say when that path would throw.
 */
const { describe, it, assert, run } = require('./harness');
const { GenericDimension } = require('../../olap-in-memory_amd/js');
const { selectionLevels, copyLevels } = require('../../olap-in-memory_amd/js/selection');

const dims = () => [
  new GenericDimension('period', 'season', ['summer', 'winter']),
  new GenericDimension('location', 'city', ['paris', 'toledo', 'tokyo']),
  new GenericDimension('kind', 'item', ['a', 'b', 'c', 'd']),
];
const plain = (levels) => ({ axis: Array.from(levels.axis), lists: levels.lists.map((l) => Array.from(l)), valid: levels.valid, count: levels.count });

// the per-cell enumeration (Cube._combinations) turned into flat positions, for comparison
function positions(dimensions, filter) {
  const options = {};
  for (const [id, value] of Object.entries(filter)) options[id] = typeof value === 'string' ? [value] : value;
  for (const d of dimensions) if (filter[d.id] === undefined) options[d.id] = d.getItems();
  let rows = [{}];
  for (const key of Object.keys(options)) {
    const next = [];
    for (const row of rows) for (const item of options[key]) next.push(Object.assign({}, row, { [key]: item }));
    rows = next;
  }
  return rows.map((coords) => dimensions.reduce((p, d) => p * d.numItems + d.getRootIndexFromRootItem(coords[d.id]), 0));
}
function expand(dimensions, levels) {
  const out = [];
  const walk = (l, digits) => {
    if (l === levels.axis.length) {
      out.push(dimensions.reduce((p, d, k) => p * d.numItems + digits[k], 0));
      return;
    }
    for (const at of levels.lists[l]) {
      const next = digits.slice();
      if (levels.axis[l] >= 0) next[levels.axis[l]] = at;
      walk(l + 1, next);
    }
  };
  walk(0, dimensions.map(() => 0));
  return out;
}

describe('selectionLevels', () => {
  it('an empty filter is every dimension in cube order', () => {
    assert.deepEqual(plain(selectionLevels(dims(), {})), { axis: [0, 1, 2], lists: [[0, 1], [0, 1, 2], [0, 1, 2, 3]], valid: true, count: 24 });
  });

  it('filter keys first, in their own order, then the unfiltered dimensions', () => {
    const d = dims();
    const filter = { kind: ['c', 'a'], period: 'winter' };
    const levels = selectionLevels(d, filter);
    assert.deepEqual(plain(levels), { axis: [2, 0, 1], lists: [[2, 0], [1], [0, 1, 2]], valid: true, count: 6 });
    assert.deepEqual(expand(d, levels), positions(d, filter));
  });

  it('a string is a one-item list, an array is taken as it is', () => {
    assert.deepEqual(plain(selectionLevels(dims(), { location: 'tokyo' })).lists[0], [2]);
    assert.deepEqual(plain(selectionLevels(dims(), { location: ['tokyo'] })).lists[0], [2]);
  });

  it('repeats are visited twice', () => {
    const d = dims();
    const filter = { location: ['paris', 'paris', 'tokyo'] };
    const levels = selectionLevels(d, filter);
    assert.deepEqual(Array.from(levels.lists[0]), [0, 0, 2]);
    assert.equal(levels.count, 3 * 2 * 4);
    assert.deepEqual(expand(d, levels), positions(d, filter));
  });

  it('a key that is not a dimension multiplies the combinations', () => {
    const d = dims();
    const filter = { colour: ['red', 'blue', 'green'], period: 'summer' };
    const levels = selectionLevels(d, filter);
    assert.deepEqual(Array.from(levels.axis), [-1, 0, 1, 2]);
    assert.equal(levels.lists[0].length, 3);
    assert.equal(levels.valid, true);
    assert.equal(levels.count, 3 * 1 * 3 * 4);
    assert.deepEqual(expand(d, levels), positions(d, filter));
  });

  it('an empty list gives no combination', () => {
    const levels = selectionLevels(dims(), { location: [] });
    assert.equal(levels.count, 0);
    assert.equal(levels.valid, true);
    assert.equal(selectionLevels(dims(), { colour: [] }).count, 0);
  });

  it('permuted nesting over random filters enumerates like the per-cell path', () => {
    const d = dims();
    let seed = 7;
    const rnd = (n) => {
      seed = (seed * 1103515245 + 12345) % 2147483648;
      return seed % n;
    };
    for (let trial = 0; trial < 200; ++trial) {
      const filter = {};
      const order = d.map((x) => x.id).sort(() => rnd(3) - 1);
      for (const id of order) {
        if (rnd(2)) continue;
        const items = d.find((x) => x.id === id).getItems();
        const list = Array.from({ length: rnd(4) }, () => items[rnd(items.length)]);
        filter[id] = list.length === 1 && rnd(2) ? list[0] : list;
      }
      if (rnd(4) === 0) filter.extra = ['x', 'y'];
      const levels = selectionLevels(d, filter);
      assert.equal(levels.valid, true);
      assert.deepEqual(expand(d, levels), positions(d, filter));
      assert.equal(levels.count, positions(d, filter).length);
    }
  });

  it('detects the filters the per-cell path throws on', () => {
    assert.equal(selectionLevels(dims(), { location: 'berlin' }).valid, false); // getPosition: no such item
    assert.equal(selectionLevels(dims(), { location: ['paris', 'berlin'] }).valid, false);
    assert.equal(selectionLevels(dims(), { location: [''] }).valid, false); // no value for all dimensions
    assert.equal(selectionLevels(dims(), { location: [null] }).valid, false);
    assert.equal(selectionLevels(dims(), { location: 3 }).valid, false); // not iterable
    assert.equal(selectionLevels(dims(), { colour: { a: 1 } }).valid, false);
    assert.equal(selectionLevels(dims(), { location: undefined }).valid, true); // undefined: all items
    assert.equal(selectionLevels(dims(), { colour: [null, ''] }).valid, true); // a free key's items are never read
  });
});

describe('copyLevels', () => {
  it('removes repeats (first occurrence kept) and drops free keys', () => {
    const d = dims();
    const filter = { kind: ['d', 'a', 'd', 'b', 'a'], colour: ['x', 'y'], location: ['tokyo', 'tokyo'] };
    const copy = copyLevels(selectionLevels(d, filter));
    assert.deepEqual(Array.from(copy.axis), [2, 1, 0]);
    assert.deepEqual(copy.lists.map((l) => Array.from(l)), [[3, 0, 1], [2], [0, 1]]);
    assert.equal(copy.count, 6);
    // the distinct cells in the order the per-cell loop first writes them
    const firstSeen = [];
    for (const p of positions(d, filter)) if (!firstSeen.includes(p)) firstSeen.push(p);
    assert.deepEqual(expand(d, copy), firstSeen);
  });

  it('an empty list (a free key included) copies nothing', () => {
    assert.equal(copyLevels(selectionLevels(dims(), { colour: [] })).count, 0);
    assert.equal(copyLevels(selectionLevels(dims(), { kind: [] })).count, 0);
  });
});

run();
