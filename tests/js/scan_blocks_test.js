'use strict';
/*
 * Cube.scan / Cube.iterateOverDimension on the device: every combination served from ONE device pass
 * (HipStore.blocksMany -> olap_store_blocks_report) against literals worked out by hand from the reference's definition
 * (src/cube.js:811-823: dice to the combination's items; iterateOverDimension then slices every other dimension to 'all',
 * which leaves a lone value as it is under every rule), and against the per-combination loop on a seeded cube of four
 * measures of mixed cell type and default.
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, HipStore, setCompactIntegers } = require('../../olap-in-memory_amd/js');

const N = Number.NaN;
const G = (id, items) => new GenericDimension(id, 'item', items);

function sameValues(x, y, where) {
  assert.equal(x.length, y.length, `${where}: length`);
  for (let i = 0; i < x.length; ++i) assert.ok(Object.is(x[i], y[i]), `${where}: [${i}] ${x[i]} !== ${y[i]}`);
}

// flat index = a * 6 + b * 2 + c
const S = [1, 0, 3, 4, 0, 6, 7, 8, 0, 10, 11, 0]; // Float32, default 0 (0: unset), rule sum
const V = [N, 1.5, 2.5, N, 4.5, 5.5, 6.5, N, 8.5, 9.5, N, 11.5]; // Float64, default NaN (NaN: unset), rule average

function literalCube() {
  const cube = new Cube([G('a', ['a1', 'a2']), G('b', ['b1', 'b2', 'b3']), G('c', ['c1', 'c2'])]);
  cube.createStoredMeasure('sm', { a: 'sum', b: 'sum', c: 'sum' }, 'float32', 0);
  cube.createStoredMeasure('av', { a: 'average', b: 'average', c: 'average' }, 'float64', N);
  cube.setData('sm', S);
  cube.setData('av', V);
  return cube;
}

const collect = (cube, method, arg) => {
  const seen = [];
  cube[method](arg, (handed, combination) => seen.push({
    combination,
    dims: handed.dimensionIds,
    s: handed.getData('sm'),
    v: handed.getData('av'),
    sObject: handed.getNestedObject('sm'),
    vObject: handed.getNestedObject('av'),
    rules: JSON.parse(JSON.stringify(handed.storedMeasuresRules)),
  }));
  return seen;
};

function checkLiterals(seen, want, dims, rules) {
  assert.equal(seen.length, want.length);
  want.forEach((w, k) => {
    const where = JSON.stringify(w.combination);
    assert.deepEqual(seen[k].combination, w.combination);
    assert.deepEqual(seen[k].dims, dims, where);
    sameValues(seen[k].s, w.s, `${where} s`);
    sameValues(seen[k].v, w.v, `${where} v`);
    assert.deepEqual(seen[k].sObject, w.sObject, `${where} s object`);
    assert.deepEqual(seen[k].vObject, w.vObject, `${where} v object`);
    assert.deepEqual(seen[k].rules, rules, where);
  });
}

const OVER_A = [
  { combination: { b: 'b1', c: 'c1' }, s: [1, 7], v: [N, 6.5], sObject: { a1: 1, a2: 7 }, vObject: { a1: N, a2: 6.5 } },
  { combination: { b: 'b1', c: 'c2' }, s: [0, 8], v: [1.5, N], sObject: { a1: 0, a2: 8 }, vObject: { a1: 1.5, a2: N } },
  { combination: { b: 'b2', c: 'c1' }, s: [3, 0], v: [2.5, 8.5], sObject: { a1: 3, a2: 0 }, vObject: { a1: 2.5, a2: 8.5 } },
  { combination: { b: 'b2', c: 'c2' }, s: [4, 10], v: [N, 9.5], sObject: { a1: 4, a2: 10 }, vObject: { a1: N, a2: 9.5 } },
  { combination: { b: 'b3', c: 'c1' }, s: [0, 11], v: [4.5, N], sObject: { a1: 0, a2: 11 }, vObject: { a1: 4.5, a2: N } },
  { combination: { b: 'b3', c: 'c2' }, s: [6, 0], v: [5.5, 11.5], sObject: { a1: 6, a2: 0 }, vObject: { a1: 5.5, a2: 11.5 } },
];
const OVER_B = [
  { combination: { a: 'a1', c: 'c1' }, s: [1, 3, 0], v: [N, 2.5, 4.5], sObject: { b1: 1, b2: 3, b3: 0 }, vObject: { b1: N, b2: 2.5, b3: 4.5 } },
  { combination: { a: 'a1', c: 'c2' }, s: [0, 4, 6], v: [1.5, N, 5.5], sObject: { b1: 0, b2: 4, b3: 6 }, vObject: { b1: 1.5, b2: N, b3: 5.5 } },
  { combination: { a: 'a2', c: 'c1' }, s: [7, 0, 11], v: [6.5, 8.5, N], sObject: { b1: 7, b2: 0, b3: 11 }, vObject: { b1: 6.5, b2: 8.5, b3: N } },
  { combination: { a: 'a2', c: 'c2' }, s: [8, 10, 0], v: [N, 9.5, 11.5], sObject: { b1: 8, b2: 10, b3: 0 }, vObject: { b1: N, b2: 9.5, b3: 11.5 } },
];
const OVER_C = [
  { combination: { a: 'a1', b: 'b1' }, s: [1, 0], v: [N, 1.5], sObject: { c1: 1, c2: 0 }, vObject: { c1: N, c2: 1.5 } },
  { combination: { a: 'a1', b: 'b2' }, s: [3, 4], v: [2.5, N], sObject: { c1: 3, c2: 4 }, vObject: { c1: 2.5, c2: N } },
  { combination: { a: 'a1', b: 'b3' }, s: [0, 6], v: [4.5, 5.5], sObject: { c1: 0, c2: 6 }, vObject: { c1: 4.5, c2: 5.5 } },
  { combination: { a: 'a2', b: 'b1' }, s: [7, 8], v: [6.5, N], sObject: { c1: 7, c2: 8 }, vObject: { c1: 6.5, c2: N } },
  { combination: { a: 'a2', b: 'b2' }, s: [0, 10], v: [8.5, 9.5], sObject: { c1: 0, c2: 10 }, vObject: { c1: 8.5, c2: 9.5 } },
  { combination: { a: 'a2', b: 'b3' }, s: [11, 0], v: [N, 11.5], sObject: { c1: 11, c2: 0 }, vObject: { c1: N, c2: 11.5 } },
];
// scan keeps every dimension, the scanned ones diced to the combination's item
const SCAN_B = [
  { combination: { b: 'b1' }, s: [1, 0, 7, 8], v: [N, 1.5, 6.5, N],
    sObject: { a1: { b1: { c1: 1, c2: 0 } }, a2: { b1: { c1: 7, c2: 8 } } }, vObject: { a1: { b1: { c1: N, c2: 1.5 } }, a2: { b1: { c1: 6.5, c2: N } } } },
  { combination: { b: 'b2' }, s: [3, 4, 0, 10], v: [2.5, N, 8.5, 9.5],
    sObject: { a1: { b2: { c1: 3, c2: 4 } }, a2: { b2: { c1: 0, c2: 10 } } }, vObject: { a1: { b2: { c1: 2.5, c2: N } }, a2: { b2: { c1: 8.5, c2: 9.5 } } } },
  { combination: { b: 'b3' }, s: [0, 6, 11, 0], v: [4.5, 5.5, N, 11.5],
    sObject: { a1: { b3: { c1: 0, c2: 6 } }, a2: { b3: { c1: 11, c2: 0 } } }, vObject: { a1: { b3: { c1: 4.5, c2: 5.5 } }, a2: { b3: { c1: N, c2: 11.5 } } } },
];
const SCAN_AC = [
  { combination: { a: 'a1', c: 'c1' }, s: [1, 3, 0], v: [N, 2.5, 4.5],
    sObject: { a1: { b1: { c1: 1 }, b2: { c1: 3 }, b3: { c1: 0 } } }, vObject: { a1: { b1: { c1: N }, b2: { c1: 2.5 }, b3: { c1: 4.5 } } } },
  { combination: { a: 'a1', c: 'c2' }, s: [0, 4, 6], v: [1.5, N, 5.5],
    sObject: { a1: { b1: { c2: 0 }, b2: { c2: 4 }, b3: { c2: 6 } } }, vObject: { a1: { b1: { c2: 1.5 }, b2: { c2: N }, b3: { c2: 5.5 } } } },
  { combination: { a: 'a2', c: 'c1' }, s: [7, 0, 11], v: [6.5, 8.5, N],
    sObject: { a2: { b1: { c1: 7 }, b2: { c1: 0 }, b3: { c1: 11 } } }, vObject: { a2: { b1: { c1: 6.5 }, b2: { c1: 8.5 }, b3: { c1: N } } } },
  { combination: { a: 'a2', c: 'c2' }, s: [8, 10, 0], v: [N, 9.5, 11.5],
    sObject: { a2: { b1: { c2: 8 }, b2: { c2: 10 }, b3: { c2: 0 } } }, vObject: { a2: { b1: { c2: N }, b2: { c2: 9.5 }, b3: { c2: 11.5 } } } },
];
const ALL_RULES = { sm: { a: 'sum', b: 'sum', c: 'sum' }, av: { a: 'average', b: 'average', c: 'average' } };
const onlyRule = (id) => ({ sm: { [id]: 'sum' }, av: { [id]: 'average' } });

describe('a 2 x 3 x 2 cube against hand-worked literals', () => {
  for (const [id, want] of [['a', OVER_A], ['b', OVER_B], ['c', OVER_C]]) {
    it(`iterateOverDimension over ${id}: one device call`, () => {
      const cube = literalCube();
      checkLiterals(collect(cube, 'iterateOverDimension', id), want, [id], onlyRule(id));
      assert.equal(HipStore.lastBlocksCalls, 1);
      checkLiterals(collect(cube, '_iterateOverDimensionPerCombination', id), want, [id], onlyRule(id));
    });
  }
  it('scan over one dimension and over two: one device call each', () => {
    const cube = literalCube();
    checkLiterals(collect(cube, 'scan', ['b']), SCAN_B, ['a', 'b', 'c'], ALL_RULES);
    assert.equal(HipStore.lastBlocksCalls, 1);
    assert.equal(HipStore.lastBatchLaunches, 2); // a Float32 measure under 0 and a Float64 one under NaN: two groups
    checkLiterals(collect(cube, 'scan', ['a', 'c']), SCAN_AC, ['a', 'b', 'c'], ALL_RULES);
    assert.equal(HipStore.lastBlocksCalls, 1);
    checkLiterals(collect(cube, '_scanPerCombination', ['b']), SCAN_B, ['a', 'b', 'c'], ALL_RULES);
    checkLiterals(collect(cube, '_scanPerCombination', ['a', 'c']), SCAN_AC, ['a', 'b', 'c'], ALL_RULES);
  });
});

// ---- the per-combination loop on a seeded [5, 4, 6] cube of four measures of mixed cell type and default
let seed = 4242;
const rnd = (n) => {
  seed = (seed * 1103515245 + 12345) % 2147483648;
  return Math.floor((seed / 2147483648) * n);
};

function seededCube() {
  seed = 4242;
  const z = G('z', ['z1', 'z2', 'z3', 'z4', 'z5', 'z6']);
  z.addAttribute('item', 'half', { z1: 'lo', z2: 'lo', z3: 'lo', z4: 'hi', z5: 'hi', z6: 'hi' });
  const cube = new Cube([G('x', ['x1', 'x2', 'x3', 'x4', 'x5']), G('y', ['y1', 'y2', 'y3', 'y4']), z]);
  const fill = (def, make) => Array.from({ length: 120 }, () => (rnd(2) === 0 ? def : make()));
  cube.createStoredMeasure('fm', { x: 'sum', y: 'sum', z: 'sum' }, 'float32', 0);
  cube.setData('fm', fill(0, () => (rnd(2000) - 1000) / 8 || 0.5));
  cube.createStoredMeasure('dm', { x: 'average', y: 'average', z: 'average' }, 'float64', N);
  cube.setData('dm', fill(N, () => [0.1, -0, 1e300, -2.5, 1 / 3][rnd(5)]));
  cube.createStoredMeasure('im', { x: 'highest', y: 'lowest', z: 'sum' }, 'int32', 0); // Float64 cells
  cube.setData('im', fill(0, () => rnd(100) - 50 || 3));
  setCompactIntegers(true);
  try {
    cube.createStoredMeasure('km', { x: 'product', z: 'highest' }, 'int32', N); // Int32 cells and a mask of their own
  } finally {
    setCompactIntegers(false);
  }
  cube.setData('km', fill(N, () => [0, -(2 ** 31), 7, -7][rnd(4)]));
  cube.createComputedMeasure('both', 'fm + im');
  return cube;
}

const IDS = ['fm', 'dm', 'im', 'km'];
const snapshot = (cube) => {
  const out = { dims: cube.dimensionIds, items: cube.dimensions.map((d) => d.getItems()), rules: JSON.parse(JSON.stringify(cube.storedMeasuresRules)), computed: cube.computedMeasureIds };
  for (const id of IDS) {
    out[`data ${id}`] = cube.getData(id);
    out[`object ${id}`] = cube.getNestedObject(id);
    out[`keys ${id}`] = Array.from(cube.getStatusMap(id).keys());
  }
  for (const id of IDS) out[`total ${id}`] = cube.getTotal(id);
  out.both = cube.getData('both');
  out.bytes = Buffer.from(cube.serialize()).toString('hex');
  for (const id of IDS) out[`byteLength ${id}`] = cube.storedMeasures[id].byteLength;
  return out;
};

function sameSnapshots(a, b, what) {
  assert.equal(a.length, b.length, what);
  a.forEach((x, k) => {
    assert.deepEqual(Object.keys(x), Object.keys(b[k]));
    for (const key of Object.keys(x)) {
      const where = `${what} #${k} ${key}`;
      if (Array.isArray(x[key]) && typeof x[key][0] === 'number') sameValues(x[key], b[k][key], where);
      else if (typeof x[key] === 'number') assert.ok(Object.is(x[key], b[k][key]), `${where}: ${x[key]} !== ${b[k][key]}`);
      else assert.deepEqual(x[key], b[k][key], where);
    }
  });
}

describe('the same as the per-combination loop on a seeded cube of four measures', () => {
  const cases = [['scan', ['x']], ['scan', ['z']], ['scan', ['x', 'z']], ['scan', ['y', 'z']], ['iterateOverDimension', 'x'], ['iterateOverDimension', 'y'], ['iterateOverDimension', 'z']];
  for (const [method, arg] of cases) {
    it(`${method}(${JSON.stringify(arg)}): getData, getNestedObject, getTotal, serialize, rules`, () => {
      const cube = seededCube();
      const onePass = [];
      cube[method](arg, (handed, combination) => onePass.push(Object.assign({ combination }, snapshot(handed))));
      assert.equal(HipStore.lastBlocksCalls, 1);
      const loop = [];
      cube[`_${method}PerCombination`](arg, (handed, combination) => loop.push(Object.assign({ combination }, snapshot(handed))));
      sameSnapshots(onePass, loop, `${method} ${arg}`);
    });
    it(`${method}(${JSON.stringify(arg)}): drillUp and dice of a handed-out cube`, () => {
      const cube = seededCube();
      const derive = (handed) => {
        const out = [];
        if (handed.dimensionIds.includes('z')) out.push(handed.drillUp('z', 'half'));
        if (handed.dimensionIds.includes('y')) out.push(handed.dice('y', 'item', ['y3', 'y1']));
        if (handed.dimensionIds.includes('x')) out.push(handed.dice('x', 'item', [handed.getDimension('x').getItems()[0]]).drillUp('x', 'all'));
        return out.map(snapshot);
      };
      const onePass = [];
      cube[method](arg, (handed) => onePass.push(...derive(handed)));
      assert.equal(HipStore.lastBlocksCalls, 1);
      const loop = [];
      cube[`_${method}PerCombination`](arg, (handed) => loop.push(...derive(handed)));
      assert.ok(onePass.length > 0);
      sameSnapshots(onePass, loop, `${method} ${arg} derived`);
    });
  }

  it('a callback that writes to the source: the remaining combinations see the write, as in the loop', () => {
    const run1 = (method) => {
      const cube = seededCube();
      const seen = [];
      cube[method]('z', (handed, combination) => {
        seen.push(handed.getData('fm'));
        if (combination.x === 'x2' && combination.y === 'y2') cube.setSingleData('fm', { x: 'x4', y: 'y1', z: 'z3' }, 4096.5);
      });
      return seen;
    };
    const onePass = run1('iterateOverDimension');
    const loop = run1('_iterateOverDimensionPerCombination');
    assert.equal(onePass.length, 20);
    onePass.forEach((row, k) => sameValues(row, loop[k], `combination ${k}`));
    assert.equal(onePass[12][2], 4096.5); // (x4, y1) is combination 3 * 4 + 0
  });
});

run();
