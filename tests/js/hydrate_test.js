'use strict';
/*
 * Cube.hydrateFromSparseNestedObject (one HipStore.setValues per call) against the per-cell walk it replaces
 * (Cube._hydrateFromSparseNestedObjectPerCell): same data, same key order, same serialize() bytes, same errors and
 * the same partial writes.  Run plain and with OLAP_DEVICES=0,0 (untracked measures split over two shards).
 */
const { describe, it, assert, run } = require('./harness');
const { Cube, GenericDimension, TimeDimension, setCompactIntegers } = require('../../olap-in-memory_amd/js');

let seed = 4242;
const rnd = (n) => {
  seed = (seed * 1103515245 + 12345) % 2147483648;
  return Math.floor((seed / 2147483648) * n);
};
const shuffled = (list) => list.map((x) => [rnd(1000), x]).sort((a, b) => a[0] - b[0]).map((p) => p[1]);

const CELL_TYPES = [
  ['float32', false],
  ['int32', false],
  ['int32', true],
  ['float64', false],
];
const RULES = [{}, { a: 'first', b: 'first' }, { a: 'last', b: 'last' }];

function dimensions(kind) {
  const items = (p, n) => Array.from({ length: n }, (_, i) => `${p}${i}`);
  if (kind === 'time') return [new TimeDimension('a', 'month', '2010-01', '2010-12'), new GenericDimension('b', 'item', items('b', 5))];
  return [new GenericDimension('a', 'item', items('a', 7)), new GenericDimension('b', 'item', items('b', 6))];
}

function makeCube(kind, type, compact, rules, def) {
  setCompactIntegers(compact);
  try {
    const cube = new Cube(dimensions(kind));
    cube.createStoredMeasure('mm', rules, type, def);
    return cube;
  } finally {
    setCompactIntegers(false);
  }
}

function leaf() {
  const r = rnd(20);
  if (r === 0) return null;
  if (r === 1) return undefined;
  if (r === 2) return 0;
  if (r === 3) return Number.NaN;
  if (r === 4) return -0;
  if (r === 5) return 1e-50;
  if (r === 6) return 3e9;
  return (rnd(40) - 20) * (rnd(2) ? 0.25 : 1);
}

// a sparse nested object over the cube's items (keys in random order) with unknown keys mixed in
function randomObject(cube) {
  const [a, b] = cube.dimensions;
  const obj = {};
  for (const x of shuffled(a.getItems().concat(['unknown']))) {
    if (rnd(3) === 0) continue;
    const inner = {};
    for (const y of shuffled(b.getItems().concat(['nope']))) if (rnd(2)) inner[y] = leaf();
    obj[x] = inner;
  }
  return obj;
}

// serialize() bytes with every NUMBER record (wire.js: tag 7, then a float32) that holds a NaN rewritten to one NaN:
// V8's DataView.setFloat32 does not write the same NaN bits on every call (a NaN default value came out as 0x7fc00000
// from one cube and 0xffffffff from the other), so only the NaN-ness of such a record is compared
function serialized(cube) {
  const bytes = Buffer.from(cube.serialize());
  for (let i = 0; i + 8 <= bytes.length; i += 4) {
    if (bytes.readUInt32LE(i) !== 7) continue;
    const v = bytes.readUInt32LE(i + 4);
    if ((v & 0x7f800000) === 0x7f800000 && (v & 0x7fffff) !== 0) bytes.writeUInt32LE(0x7fc00000, i + 4);
  }
  return bytes;
}

function assertSame(a, b) {
  assert.deepEqual(a.getData('mm'), b.getData('mm'));
  assert.deepEqual(Array.from(a.getStatusMap('mm').keys()), Array.from(b.getStatusMap('mm').keys()));
  const x = serialized(a);
  const y = serialized(b);
  if (!x.equals(y)) {
    let at = 0;
    while (at < Math.min(x.length, y.length) && x[at] === y[at]) ++at;
    const window = (buf) => buf.slice(Math.max(0, at - 32), at + 32).toString('hex');
    throw new Error(`serialize() differs at byte ${at} of ${x.length} / ${y.length}: ${window(x)} vs ${window(y)}`);
  }
}

// runs fn on the batched cube and perCell on the other; both must throw the same message (or neither)
function both(a, b, fn, perCell) {
  let ea = null;
  let eb = null;
  try {
    fn(a);
  } catch (e) {
    ea = e.message;
  }
  try {
    perCell(b);
  } catch (e) {
    eb = e.message;
  }
  assert.equal(ea, eb);
  assertSame(a, b);
  return ea;
}

describe('hydrateFromSparseNestedObject in one setValues', () => {
  for (const kind of ['generic', 'time']) {
    for (const [type, compact] of CELL_TYPES) {
      for (const rules of RULES) {
        for (const def of [0, Number.NaN]) {
          const name = `${kind} ${type}${compact ? ' (compact)' : ''} ${JSON.stringify(rules)} default ${def}`;
          it(name, () => {
            const a = makeCube(kind, type, compact, rules, def);
            const b = makeCube(kind, type, compact, rules, def);
            for (let round = 0; round < 3; ++round) {
              const obj = randomObject(a);
              both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', obj), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', obj));
            }
          });
        }
      }
    }
  }

  it('one setValues and no setValue for a numeric object', () => {
    const cube = makeCube('generic', 'float32', false, {}, 0);
    const store = cube.storedMeasures.mm;
    const calls = { setValue: 0, setValues: 0 };
    for (const method of ['setValue', 'setValues']) {
      const original = store[method];
      store[method] = function spy(...args) {
        calls[method] += 1;
        return original.apply(this, args);
      };
    }
    cube.hydrateFromSparseNestedObject('mm', { a3: { b1: 1, b4: 2 }, a0: { b5: 3, b0: null } });
    assert.deepEqual(calls, { setValue: 0, setValues: 1 });
    assert.deepEqual(Array.from(cube.getStatusMap('mm').keys()), [5, 19, 22]);
  });

  it('too-shallow and too-deep objects', () => {
    for (const rules of RULES) {
      const a = makeCube('generic', 'float32', false, rules, Number.NaN);
      const b = makeCube('generic', 'float32', false, rules, Number.NaN);
      const shallow = { a1: 5, a2: { b1: 2 } };
      both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', shallow), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', shallow));
      const deep = { a1: { b1: { x: 1 } }, a2: { b2: 3 } };
      both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', deep), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', deep));
    }
  });

  it('non-number leaves take the per-cell path (coercion and its throws in place)', () => {
    const a = makeCube('generic', 'float64', false, { a: 'last', b: 'last' }, 0);
    const b = makeCube('generic', 'float64', false, { a: 'last', b: 'last' }, 0);
    const odd = { a4: { b2: 1, b0: '7', b1: true }, a1: { b3: 2 } };
    both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', odd), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', odd));
    const throwing = { a2: { b2: 4 }, a5: { b1: { valueOf() { throw new Error('no number here'); } } }, a6: { b0: 9 } };
    const message = both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', throwing), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', throwing));
    assert.equal(message, 'no number here');
    assert.equal(a.getData('mm')[2 * 6 + 2], 4);
  });

  it('a walk that throws halfway leaves the prefix written', () => {
    const a = makeCube('time', 'float32', false, { a: 'first', b: 'first' }, 0);
    const b = makeCube('time', 'float32', false, { a: 'first', b: 'first' }, 0);
    const broken = { '2010-05': { b3: 1, b1: 2 }, get '2010-02'() { throw new Error('walk broke'); }, '2010-09': { b0: 3 } };
    const message = both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', broken), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', broken));
    assert.equal(message, 'walk broke');
    assert.deepEqual(Array.from(a.getStatusMap('mm').keys()), [4 * 5 + 3, 4 * 5 + 1]);
  });

  it('offsets outside the store and unknown measures fail as per cell', () => {
    const a = makeCube('generic', 'float32', false, {}, 0);
    const b = makeCube('generic', 'float32', false, {}, 0);
    const obj = { a0: { b1: 1 }, a6: { b5: 2 } };
    assert.ok(both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', obj, 1), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', obj, 1)) !== null);
    assert.ok(both(a, b, (c) => c.hydrateFromSparseNestedObject('zz', obj), (c) => c._hydrateFromSparseNestedObjectPerCell('zz', obj)) !== null);
    both(a, b, (c) => c.hydrateFromSparseNestedObject('mm', {}), (c) => c._hydrateFromSparseNestedObjectPerCell('mm', {}));
  });

  it('HipStore.setValues validates its indexes before the device', () => {
    const cube = makeCube('generic', 'float32', false, {}, 0);
    const store = cube.storedMeasures.mm;
    assert.throws(() => store.setValues([1, -1], [1, 2]), /not an integer >= 0/);
    assert.throws(() => store.setValues([1.5], [1]), /not an integer >= 0/);
    assert.throws(() => store.setValues([1, 42], [1, 2]), /entry 1: cell index 42 out of bounds/);
    assert.throws(() => store.setValues([1, 2], [1]), /2 indexes, 1 values/);
    assert.deepEqual(Array.from(cube.getStatusMap('mm').keys()), []);
  });
});

run();
