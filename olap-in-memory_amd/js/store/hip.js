'use strict';
/*
 * HipStore — drop-in for the reference's InMemoryStore (/root/reference/src/store/in-memory.js)
 * whose cells live in MI355X HBM.  Same constructor, members and error messages as the members
 * `Cube` touches (SURVEY.md §8(b)): size, byteLength, total, data (get/set), clone, getValue,
 * setValue, fill, drillUp, drillDown, dice, reorder, load, _type, _defaultValue, _dataMap.
 *
 * This class only turns dimension objects into the small integer tables the C ABI takes
 * (include/olap_hip.h) and forwards; all cell work happens in the HIP kernels.
 */
const backend = require('../backend');
const { toBuffer, fromBuffer } = require('../wire');

const TYPE_CODE = { int32: 0, uint32: 1, float32: 2, float64: 3 };
const TYPE_NAME = ['int32', 'uint32', 'float32', 'float64'];
const BYTES = { int32: 4, uint32: 4, float32: 4, float64: 8 };
const TYPED_ARRAY = { int32: Int32Array, uint32: Uint32Array, float32: Float32Array, float64: Float64Array };

/**
 * The element type of the device cells of a measure DECLARED `type`.  The reference's Map holds plain
 * float64 numbers whatever the declared type and coerces only in serialize() (in-memory.js:77-92): an
 * int32 `average` of 7 and 8 is 7.5 until then, a uint32 sum may pass 2^32.  Integer measures therefore
 * live in Float64 cells (8 bytes per cell) and give the reference's values exactly; the declared type
 * still decides byteLength (:15), the remainder rule of drillDown (:343) and the serialized form.
 * backend.setCompactIntegers(true) (or OLAP_COMPACT_INT=1) stores them as 4-byte Int32 / Uint32 cells
 * instead — half the memory and traffic, values coerced after every operation.  Float32 measures are
 * Float32 cells (the tolerance the port states: 1e-5 relative).
 */
const cellTypeOf = (type) => ((type === 'int32' || type === 'uint32') && !backend.compactIntegers() ? 'float64' : type);

const lengthsOf = (dimensions) => {
  const out = new Uint32Array(dimensions.length);
  for (let i = 0; i < dimensions.length; ++i) out[i] = dimensions[i].numItems;
  return out;
};

// A dimension's index map as the Uint32Array the addon takes.  GenericDimension hands out its own Uint32Array (used as it
// is: the addon reads it during the call and keeps nothing); TimeDimension a cached plain Array, converted once per array
// (Uint32Array.from walks the iterator protocol: ~1 us per 10 items on Node 12, per dimension, per call).
const convertedMaps = new WeakMap();
const asU32 = (map) => {
  if (map instanceof Uint32Array) return map;
  let typed = convertedMaps.get(map);
  if (typed === undefined || typed.length !== map.length) {
    typed = new Uint32Array(map.length);
    for (let i = 0; i < map.length; ++i) typed[i] = map[i];
    convertedMaps.set(map, typed);
  }
  return typed;
};

// Array.from(typedArray) walks the iterator protocol (60 ms for 5e5 cells on Node 12); index loops are 20x faster
const toPlainArray = (typed) => {
  const out = new Array(typed.length);
  for (let i = 0; i < typed.length; ++i) out[i] = typed[i];
  return out;
};
const toFloat64 = (values, unset) => {
  const out = new Float64Array(values.length);
  for (let i = 0; i < values.length; ++i) {
    const v = values[i];
    out[i] = v === undefined || v === null ? unset : Number(v);
  }
  return out;
};

/** Read-only view with the Map methods the reference's callers use on `_dataMap`. */
class CellMapView {
  constructor(store) {
    this._store = store;
  }

  get size() {
    const host = this._store._hostCells;
    if (host) {
      let n = 0;
      for (let i = 0; i < host.length; ++i) if (this._store._hostIsSet(i)) ++n;
      return n;
    }
    return this._store._whole.countSet();
  }

  has(index) {
    if (this._store._hostHolds(index)) return this._store._hostIsSet(index);
    return this._store._native.getValue(index) !== undefined;
  }

  get(index) {
    if (this._store._hostHolds(index)) return this._store._hostIsSet(index) ? this._store._hostCells[index] : undefined;
    return this._store._native.getValue(index);
  }

  *keys() {
    const host = this._store._hostCells;
    if (host) {
      // (an untracked store lists its set cells in ascending index order)
      for (let i = 0; i < host.length; ++i) if (this._store._hostIsSet(i)) yield i;
      return;
    }
    for (const k of this._store._whole.getKeys()) yield k;
  }

  *values() {
    if (this._store._hostCells) {
      for (const [, v] of this.entries()) yield v;
      return;
    }
    const whole = this._store._whole;
    const data = whole.getDataF64();
    for (const k of whole.getKeys()) yield data[k];
  }

  *entries() {
    const host = this._store._hostCells;
    if (host) {
      for (let i = 0; i < host.length; ++i) if (this._store._hostIsSet(i)) yield [i, host[i]];
      return;
    }
    const whole = this._store._whole;
    const data = whole.getDataF64();
    for (const k of whole.getKeys()) yield [k, data[k]];
  }

  [Symbol.iterator]() {
    return this.entries();
  }
}

/**
 * Of two new items naming the same old item only the LAST receives the cells (the reference builds
 * `new Map(newItems.map((item, i) => [oldIdx, i]))`, in-memory.js:219-224): earlier ones become -1.
 */
function effectiveSelection(sel) {
  const last = new Map();
  sel.forEach((old, j) => {
    if (old >= 0) last.set(old, j);
  });
  return Int32Array.from(sel, (old, j) => (old >= 0 && last.get(old) === j ? old : -1));
}

/**
 * A pending selection keeps every dimension of its SOURCE store; the cube may meanwhile have
 * dropped dimensions that were reduced to one item (slice = dice to one item + removeDimension).
 * Returns, for each dimension the caller still sees, its position among the pending ones — the
 * others are the dropped single-item dimensions — or null when the extents do not line up.
 */
function visibleDims(pending, lengths) {
  const at = [];
  let v = 0;
  for (let d = 0; d < pending.midLen.length; ++d) {
    if (v < lengths.length && pending.midLen[d] === lengths[v]) at[v++] = d;
    else if (pending.midLen[d] !== 1) return null;
  }
  return v === lengths.length ? at : null;
}

/**
 * The tables of a dice, the same for every measure of a cube: per dimension the old item of each new item (-1: none),
 * the new lengths and the new size.
 */
function diceTables(oldDimensions, newDimensions) {
  const sel = newDimensions.map((dim, i) => {
    const position = oldDimensions[i].getItemsToIdx();
    return Int32Array.from(dim.getItems(), (item) => (position[item] === undefined ? -1 : position[item]));
  });
  const midLen = lengthsOf(newDimensions);
  return { oldLen: lengthsOf(oldDimensions), midLen, size: midLen.reduce((n, l) => n * l, 1), sel: sel.map(effectiveSelection) };
}

/**
 * The pending selections among `stores` that can leave together, grouped by selection: measures diced by one
 * HipStore.diceMany call hold the SAME table objects, so a group is an identity comparison.  `eligible(store)` narrows
 * further.  Returns [[index, ...], ...] of the groups of two or more; sources are whole on one device and untracked.
 */
function pendingGroups(stores, eligible = () => true) {
  const groups = new Map();
  stores.forEach((store, i) => {
    const p = store._pending;
    if (!p || !wholeUntracked(p.source) || !eligible(store)) return;
    const group = groups.get(p.sel);
    if (group === undefined) groups.set(p.sel, [i]);
    else if (stores[group[0]]._pending.oldLen === p.oldLen && stores[group[0]]._pending.midLen === p.midLen) group.push(i);
  });
  return Array.from(groups.values()).filter((group) => group.length >= 2);
}

/**
 * Calls `native[method](...args)`.  A sharded measure answers in place whatever leaves its outermost
 * dimension alone (and the roll-up of that dimension itself: one collective); for the rest the C ABI
 * refuses with a message starting "sharded:" (include/olap_hip.h) and the measure is gathered onto one
 * device first — same result, one copy more.
 */
function onShards(native, method, args) {
  if (!native.isSharded) return native[method](...args);
  try {
    return native[method](...args);
  } catch (e) {
    if (!/^sharded:/.test(e.message)) throw e;
    return native.gather()[method](...args);
  }
}

/** his item index -> my item index (-1: an item I do not have), per dimension (in-memory.js:140-150) */
function loadTables(myDimensions, hisDimensions) {
  return hisDimensions.map((dim, i) => {
    const position = myDimensions[i].getItemsToIdx();
    return Int32Array.from(dim.getItems(), (item) => (position[item] === undefined ? -1 : position[item]));
  });
}

/** Whether an addon store is held whole on one device and untracked: what the calls over several measures take. */
const wholeUntracked = (native) => !!native && !native.isSharded && !native.orderTracked;
/**
 * The addon store that decides it for a HipStore.  heldStore: after materializeMany — a selection that is still pending
 * (alone in its group, or over a sharded source) gives null, like cells still on the host, and the measure goes one by
 * one.  sourceStore: before it — a pending selection answers for its source.
 */
const heldStore = (store) => (store._pending ? null : store._nativeStore);
const sourceStore = (store) => (store._pending ? store._pending.source : store._nativeStore);

/**
 * The last step of drillUpMany, drillDownMany and reorderMany: the measures without a result in `out` that are held whole
 * and untracked (and `eligible(i)`) go to the device together when there are two or more — `call(addon stores)` gives the
 * new addon stores, wrapped back in place — and the rest one by one through `single(store, i)`.
 */
function togetherThenSingly(stores, out, eligible, call, single) {
  const together = [];
  stores.forEach((store, i) => {
    if (!out[i] && wholeUntracked(heldStore(store)) && eligible(i)) together.push(i);
  });
  if (together.length >= 2) {
    const natives = call(together.map((i) => stores[i]._nativeStore), together);
    together.forEach((i, j) => {
      out[i] = stores[i]._wrap(natives[j]);
    });
  }
  stores.forEach((store, i) => {
    if (!out[i]) out[i] = single(store, i);
  });
  return out;
}

/** old item -> new item per dimension of a roll-up, and how many dimensions such maps actually roll up */
const drillUpMaps = (oldDimensions, newDimensions) => newDimensions.map((dim, i) => asU32(oldDimensions[i].getGroupIndexFromRootIndexMap(dim.rootAttribute)));
const rolledUp = (maps, newDimensions) => maps.filter((map, i) => map.length !== newDimensions[i].numItems || map.some((g, k) => g !== k)).length;

/** A roll-up over the dimensions the cube sees (`at`: visibleDims) on those of the pending selection `p`: the ones the cube has dropped keep their single item */
function rollUpOfPending(p, at, newDimensions, maps) {
  const newLen = Uint32Array.from(p.midLen, () => 1);
  const allMaps = Array.from(p.midLen, () => Uint32Array.of(0));
  at.forEach((d, v) => {
    newLen[d] = newDimensions[v].numItems;
    allMaps[d] = maps[v];
  });
  return { newLen, allMaps };
}

/** the code Store.drillDown takes: sum or a copy, and the remainder rule of the DECLARED type (in-memory.js:343), whatever the cells are (OLAP_DRILLDOWN_INTEGER_MEASURE) */
const drillDownCode = (store, method) => (method === undefined || method === 'sum' ? 0 : 4) | (store._type === 'int32' || store._type === 'uint32' ? 0x100 : 0);

const reorderPerm = (oldDimensions, newDimensions) => Int32Array.from(newDimensions, (dim) => oldDimensions.indexOf(dim));

class HipStore {
  /**
   * `native` is the addon Store, or — for the result of dice() — a pending selection
   * `{ source, oldLen, sel }` that is only materialised when cells are actually needed: a drillUp
   * that follows (slice, removeDimension, drillUp after dice) runs fused and never writes the diced
   * intermediate cube (K5, DESIGN.md §3).  Or — for the cubes Cube.scan / iterateOverDimension hand out — host-resident
   * cells `{ host: Float64Array, cells }`: the `size` cells with the default in unset ones, as blocksMany brought them back,
   * of a source whose device cells are of type `cells`.  Reads answer from the array; the first operation that needs the
   * device creates the store (the _native getter) and the measure is an ordinary one from then on (K11, DESIGN.md §3).
   */
  constructor(size, type = 'float32', defaultValue = Number.NaN, native = undefined, lengths = undefined) {
    // same checks, order and messages as in-memory.js:56-60
    if (!Number.isNaN(defaultValue) && defaultValue !== 0) throw new Error('Invalid default value, only NaN and 0 are supported');
    if (!Object.prototype.hasOwnProperty.call(TYPE_CODE, type)) throw new Error('Invalid type');
    this._size = size;
    this._type = type;
    this._defaultValue = defaultValue;
    this._pending = null;
    this._lent = false; // a pending dice elsewhere still reads this store's device buffer
    this._host = null;
    this._writes = 0; // bumped whenever this store is handed out for writing (_writable): Cube.scan watches it
    if (native && native.host) {
      if (native.host.length !== size) throw new Error(`value length is invalid: ${size} !== ${native.host.length}`);
      this._host = native.host;
      this._nativeStore = null;
      this._cells = native.cells;
    } else if (native && native.source) {
      this._pending = native;
      this._nativeStore = null;
      this._cells = TYPE_NAME[native.source.dtype];
    } else {
      this._nativeStore = native || HipStore._create(size, cellTypeOf(type), defaultValue, lengths);
      this._cells = TYPE_NAME[this._nativeStore.dtype];
    }
    this._dataMap = new CellMapView(this);
  }

  /**
   * A new device store.  When a device list is set (backend.setDevices / OLAP_DEVICES) and the caller says
   * how the cells are laid out (`lengths`, what Cube passes), the measure is split along dimension 0 over
   * those devices; the reference's bare `new Store(size, type, default)` stays on one device.
   */
  static _create(size, type, defaultValue, lengths) {
    const addon = backend.load();
    const def = Number.isNaN(defaultValue) ? 1 : 0;
    if (HipStore.splits(lengths)) return new addon.ShardedStore(Uint32Array.from(lengths), TYPE_CODE[type], def);
    return new addon.Store(size, TYPE_CODE[type], def);
  }

  /** Whether a new store laid out as `lengths` is split over the devices of the list (see _create). */
  static splits(lengths) {
    const world = backend.load().shardWorld();
    return world >= 2 && !!lengths && lengths.length >= 1 && lengths[0] >= world;
  }

  /**
   * The device store (one device, or sharded); a pending dice is executed on first use, and host-resident cells are
   * uploaded into a new store of the source's cell type and default — the store the per-combination path would have made.
   */
  get _native() {
    if (!this._nativeStore) {
      if (this._host) {
        const native = new (backend.load().Store)(this._size, TYPE_CODE[this._cells], Number.isNaN(this._defaultValue) ? 1 : 0);
        native.setData(this._host);
        this._nativeStore = native;
        this._host = null;
        return native;
      }
      const p = this._pending;
      this._nativeStore = onShards(p.source, 'dice', [p.oldLen, p.midLen, p.sel]);
      this._pending = null;
    }
    return this._nativeStore;
  }

  /** Runs a pending dice (or uploads host-resident cells) now: what the first use of `_native` does. */
  _materialize() {
    return this._native;
  }

  /** The host-resident cells while no device store exists yet (null otherwise). */
  get _hostCells() {
    return this._nativeStore ? null : this._host;
  }

  _hostHolds(index) {
    return this._hostCells !== null && Number.isInteger(index) && index >= 0 && index < this._size;
  }

  /** What the `data` setter would make of host cell `index`: set iff its value is not the default. */
  _hostIsSet(index) {
    const v = this._host[index];
    return Number.isNaN(this._defaultValue) ? !Number.isNaN(v) : v !== 0;
  }

  /**
   * Keep the reference Map's INSERTION order for this measure (in-memory.js:298): `first` / `last`, `_dataMap.keys()`
   * and serialize() then answer exactly as the reference does after out-of-order setValue calls, roll-ups of sparse
   * cubes, permuting dices and reorders.  Costs a second pass per operation once the order leaves the flat index;
   * Cube turns it on for measures with a `first` / `last` rule.  Results of operations inherit it.  (One device only:
   * a sharded measure is gathered first.)
   */
  trackOrder(on = true) {
    if (this._native.isSharded) this._nativeStore = this._native.gather();
    this._writable.trackOrder(on);
    return this;
  }

  get orderTracked() {
    const native = this._pending ? this._pending.source : this._nativeStore;
    return native && !native.isSharded ? native.orderTracked : 0;
  }

  /** The measure as ONE device store: a sharded measure is gathered (what the shards cannot answer in place). */
  get _whole() {
    const native = this._native;
    return native.isSharded ? native.gather() : native;
  }

  /**
   * The device store for writing.  Pending dices read their source lazily, and the reference's
   * dice() returns an independent copy: a store whose buffer has been lent out writes to a fresh
   * copy and leaves the lent one to its readers (copy-on-write, at most once per lending).
   */
  get _writable() {
    ++this._writes;
    const native = this._native;
    if (this._lent) {
      this._nativeStore = native.clone();
      this._lent = false;
    }
    return this._nativeStore;
  }

  _wrap(native) {
    return new HipStore(native.size, this._type, this._defaultValue, native);
  }

  get size() {
    return this._size;
  }

  get byteLength() {
    return this._size * (BYTES[this._type] || 1);
  }

  get total() {
    return this._native.total();
  }

  /** Dense plain Array, default value in unset cells (in-memory.js:30-37). */
  get data() {
    if (this._hostCells) return toPlainArray(this._host);
    return toPlainArray(this._native.getDataF64());
  }

  set data(values) {
    if (this._size !== values.length) throw new Error(`value length is invalid: ${this._size} !== ${values.length}`);
    const widened = this._cells === 'float64' && (values instanceof Int32Array || values instanceof Uint32Array || values instanceof Float32Array);
    if (ArrayBuffer.isView(values) && !(values instanceof Float64Array) && (values.constructor === TYPED_ARRAY[this._cells] || widened) &&
        !this._native.isSharded) {
      // a typed array of the store's own element type: no conversion; a narrower one into Float64 cells: widened by the addon
      this._writable.setData(values);
      return;
    }
    const d = this._defaultValue;
    // undefined / null unset the cell, exactly like the default value does (in-memory.js:122-133)
    this._writable.setData(toFloat64(values, d));
  }

  clone() {
    return this._wrap(this._native.clone());
  }

  getValue(index) {
    if (this._hostHolds(index)) return this._host[index];
    const v = this._native.getValue(index);
    return v === undefined ? this._defaultValue : v;
  }

  setValue(index, value) {
    this._writable.setValue(index, value);
  }

  /**
   * setValue(indexes[i], values[i]) for every i, in list order, as one device call: the same values, mask and key
   * order.  A null or undefined value unsets its cell; other values are coerced to numbers as setValue does.
   */
  setValues(indexes, values) {
    const n = indexes.length;
    if (values.length !== n) throw new Error(`setValues: ${n} indexes, ${values.length} values`);
    const idx = Float64Array.from(indexes);
    const vals = new Float64Array(n);
    let nulls;
    for (let i = 0; i < n; ++i) {
      const v = values[i];
      if (v === null || v === undefined) {
        if (nulls === undefined) nulls = new Uint8Array(n);
        nulls[i] = 1;
      } else {
        vals[i] = +v;
      }
    }
    this._writable.setValues(idx, vals, nulls);
  }

  fill(value) {
    if (value === undefined || value === null) this._writable.fill(this._defaultValue);
    else this._writable.fill(value);
  }

  /**
   * Every marginal of this measure (src/cube.js:421-440) as the flat extended cube: one more item, 'all', at
   * the end of every dimension.  `methods[d]` is the measure's rule for dimension d (default 'sum').
   */
  totals(dimensions, methods) {
    const addon = backend.load();
    const codes = Int32Array.from(dimensions, (_, d) => addon.methodFromName(methods[d])); // throws 'Unsupported aggregation method: <m>'
    return this._whole.totals(lengthsOf(dimensions), codes);
  }

  /** in-memory.js:265-334 */
  drillUp(oldDimensions, newDimensions, method = 'sum') {
    const code = backend.load().methodFromName(method); // throws 'Unsupported aggregation method: <m>'
    const maps = drillUpMaps(oldDimensions, newDimensions);
    const at = this._pending && !this._pending.source.isSharded ? visibleDims(this._pending, lengthsOf(oldDimensions)) : null;
    if (at) {
      const rolled = rolledUp(maps, newDimensions);
      const p = this._pending;
      // every group has exactly its own single member (e.g. the roll-up to 'all' of a dimension that
      // a slice diced down to one item): the cells do not change, the selection stays pending and
      // keeps composing — slice(...).dice(...).drillUp(...) becomes ONE launch over the source cube
      if (rolled === 0) return new HipStore(this._size, this._type, this._defaultValue, { source: p.source, oldLen: p.oldLen, midLen: p.midLen, sel: p.sel });
      if (rolled <= 1) {
        const { newLen, allMaps } = rollUpOfPending(p, at, newDimensions, maps);
        return this._wrap(p.source.diceDrillUp(p.oldLen, p.midLen, newLen, p.sel, allMaps, code));
      }
    }
    return this._wrap(onShards(this._native, 'drillUp', [lengthsOf(oldDimensions), lengthsOf(newDimensions), maps, code]));
  }

  /**
   * drillUp of the stored measures of one cube, each by its own rule — what Cube.drillUp asks of every stored measure
   * in turn (src/cube.js:1012-1020).  Measures held whole on one device go to the device TOGETHER (addon drillUpMulti ->
   * olap_store_drillup_multi: one launch for the measures that share cell type and default — even with different rules
   * when the roll-up streams whole rows — one launch per rule otherwise); the others (pending selections, sharded or
   * order-tracking measures, a lone measure) take drillUp one by one.  Returns the new stores in the order given.
   */
  static drillUpMany(stores, oldDimensions, newDimensions, methods) {
    const out = new Array(stores.length);
    const lengths = lengthsOf(oldDimensions);
    let launches = 0;
    // pending selections that share one selection (diceMany): a roll-up of one dimension runs fused over the SOURCE cubes
    // (K5), all measures behind one call (addon diceDrillUpMulti -> olap_store_dice_drillup_multi: one launch per rule and
    // cell type).  A roll-up that changes nothing stays pending, measure by measure, as drillUp leaves it.
    const fusable = pendingGroups(stores, (store) => visibleDims(store._pending, lengths) !== null);
    if (fusable.length > 0) {
      const addon = backend.load();
      const maps = drillUpMaps(oldDimensions, newDimensions);
      const rolled = rolledUp(maps, newDimensions);
      for (const group of rolled === 1 ? fusable : []) {
        const p = stores[group[0]]._pending;
        const { newLen, allMaps } = rollUpOfPending(p, visibleDims(p, lengths), newDimensions, maps);
        const codes = Int32Array.from(group, (i) => addon.methodFromName(methods[i] === undefined ? 'sum' : methods[i])); // throws 'Unsupported aggregation method: <m>'
        const launchesOut = new Int32Array(1);
        const natives = addon.diceDrillUpMulti(group.map((i) => stores[i]._pending.source), codes, p.oldLen, p.midLen, newLen, p.sel, allMaps, launchesOut);
        group.forEach((i, j) => {
          out[i] = stores[i]._wrap(natives[j]);
        });
        launches += launchesOut[0];
      }
      // more than one dimension rolled up: no fused form, the measures are diced together first
      if (rolled > 1) {
        HipStore.materializeMany(stores);
        launches += HipStore.lastBatchLaunches;
      }
    }
    // pending selections whose dimensions no longer line up with the cube's cannot fuse either
    const unfusable = stores.filter((store, i) => !out[i] && store._pending && !store._pending.source.isSharded && visibleDims(store._pending, lengths) === null);
    if (unfusable.length >= 2) {
      HipStore.materializeMany(unfusable);
      launches += HipStore.lastBatchLaunches;
    }
    HipStore.lastBatchLaunches = launches;
    return togetherThenSingly(stores, out, () => true, (natives, together) => {
      const addon = backend.load();
      const codes = Int32Array.from(together, (i) => addon.methodFromName(methods[i] === undefined ? 'sum' : methods[i])); // throws 'Unsupported aggregation method: <m>'
      return addon.drillUpMulti(natives, codes, lengthsOf(oldDimensions), lengthsOf(newDimensions), drillUpMaps(oldDimensions, newDimensions));
    }, (store, i) => store.drillUp(oldDimensions, newDimensions, methods[i]));
  }

  /** in-memory.js:336-430 — any method other than 'sum' copies the parent value (:421-423) */
  drillDown(oldDimensions, newDimensions, method = 'sum', distributions = null) {
    const maps = oldDimensions.map((dim, i) => asU32(newDimensions[i].getGroupIndexFromRootIndexMap(dim.rootAttribute)));
    const weights = distributions ? toFloat64(distributions, Number.NaN) : null;
    return this._wrap(onShards(this._native, 'drillDown', [lengthsOf(oldDimensions), lengthsOf(newDimensions), maps, drillDownCode(this, method), weights]));
  }

  /**
   * drillDown of the stored measures of one cube, each by its own rule — what Cube.drillDown and Cube.addDimension ask
   * of every stored measure in turn.  Measures held whole on one device, untracked and without a distribution go to the
   * device TOGETHER (addon drillDownMulti -> olap_store_drilldown_multi: one launch for up to 8 measures that share cell
   * type, default, sum-or-copy and the integer remainder rule); the others take drillDown one by one.  Pending
   * selections are diced together first (materializeMany).  Returns the new stores in the order given.
   */
  static drillDownMany(stores, oldDimensions, newDimensions, methods, distributionsPerStore = []) {
    const out = new Array(stores.length);
    HipStore.materializeMany(stores); // (leaves its launches in HipStore.lastBatchLaunches)
    return togetherThenSingly(stores, out, (i) => !distributionsPerStore[i], (natives, together) => {
      const maps = oldDimensions.map((dim, i) => asU32(newDimensions[i].getGroupIndexFromRootIndexMap(dim.rootAttribute)));
      const codes = Int32Array.from(together, (i) => drillDownCode(stores[i], methods[i]));
      const launchesOut = new Int32Array(1);
      const made = backend.load().drillDownMulti(natives, codes, lengthsOf(oldDimensions), lengthsOf(newDimensions), maps, launchesOut);
      HipStore.lastBatchLaunches += launchesOut[0];
      return made;
    }, (store, i) => store.drillDown(oldDimensions, newDimensions, methods[i], distributionsPerStore[i]));
  }

  /** in-memory.js:213-263 — the new dimensions' item ORDER decides where cells land */
  dice(oldDimensions, newDimensions) {
    return this._diceWith(diceTables(oldDimensions, newDimensions), new Map());
  }

  /**
   * dice by ready-made tables (diceTables).  `compositions`: what the tables give on top of a pending selection, by that
   * selection — measures that share one (diceMany) compose it once and go on sharing the result.
   */
  _diceWith(tables, compositions) {
    const { oldLen, midLen, size, sel } = tables;
    const at = this._pending ? visibleDims(this._pending, oldLen) : null;
    if (at) {
      // dice of a pending dice: compose the selections, still nothing is materialised
      const p = this._pending;
      let composed = compositions.get(p.sel);
      if (composed === undefined || composed.from !== p.midLen) {
        const all = p.sel.slice();
        const allLen = Uint32Array.from(p.midLen);
        at.forEach((d, v) => {
          all[d] = Int32Array.from(sel[v], (j) => (j < 0 ? -1 : p.sel[d][j]));
          allLen[d] = midLen[v];
        });
        composed = { from: p.midLen, midLen: allLen, sel: all };
        compositions.set(p.sel, composed);
      }
      return new HipStore(size, this._type, this._defaultValue, { source: p.source, oldLen: p.oldLen, midLen: composed.midLen, sel: composed.sel });
    }
    const source = this._native; // (materialises a pending selection whose dimensions no longer line up)
    // a tracked measure: the diced store has an order of its own that the next operation must see
    if (!source.isSharded && source.orderTracked) return this._wrap(source.dice(oldLen, midLen, sel));
    this._lent = true;
    return new HipStore(size, this._type, this._defaultValue, { source, oldLen, midLen, sel });
  }

  /**
   * dice of the stored measures of one cube — what Cube._diced asks of every stored measure in turn: the selection is
   * computed once and every pending store this creates holds the SAME table objects, so that what follows (drillUpMany,
   * materializeMany) finds the measures that can leave in one launch by comparing identities.  Nothing is launched here
   * (selections stay pending, as dice() leaves them); tracked measures are diced at once, as dice() does.
   */
  static diceMany(stores, oldDimensions, newDimensions) {
    const tables = diceTables(oldDimensions, newDimensions);
    const compositions = new Map();
    // (selections whose dimensions no longer line up with the cube's are diced first — together: the only launches here)
    HipStore.materializeMany(stores.filter((store) => store._pending && !visibleDims(store._pending, tables.oldLen)));
    return stores.map((store) => store._diceWith(tables, compositions));
  }

  /**
   * Runs the pending selections among `stores` that share one selection (diceMany) as ONE device call per group (addon
   * diceMulti -> olap_store_dice_multi: one launch for up to 8 measures of one cell type and default) and installs the
   * results, so that an operation that needs the cells of every measure does not dice them one by one.  A selection on
   * its own, or over a sharded source, stays pending.
   */
  static materializeMany(stores) {
    let launches = 0;
    const groups = pendingGroups(stores);
    if (groups.length > 0) {
      const addon = backend.load();
      for (const group of groups) {
        const p = stores[group[0]]._pending;
        const launchesOut = new Int32Array(1);
        const natives = addon.diceMulti(group.map((i) => stores[i]._pending.source), p.oldLen, p.midLen, p.sel, launchesOut);
        group.forEach((i, j) => {
          stores[i]._nativeStore = natives[j];
          stores[i]._pending = null;
        });
        launches += launchesOut[0];
      }
    }
    HipStore.lastBatchLaunches = launches;
  }

  /**
   * getTotalForDimensionItems (src/cube.js:679-707) over a selection in nesting order (./selection.js: `axis` per level,
   * a cube dimension or -1, and Int32Array `lists` of item indices, -1 = a cell that does not exist): the float64 sum of
   * getValue from +0 in that order, bit for bit.  A pending dice composes the levels through its selection instead of
   * being materialised.  HipStore.lastSelectPath says what ran: 'device' (the certified order-free reduction) or
   * 'sequential' (the values gathered in nesting order and added on the host).
   */
  selectTotal(lengths, levels) {
    const pathOut = new Int32Array(1);
    let native = null;
    let lens = lengths;
    let axis = levels.axis;
    let lists = levels.lists;
    const at = this._pending ? visibleDims(this._pending, lengths) : null;
    if (at) {
      const p = this._pending;
      const dropped = [];
      for (let d = 0; d < p.midLen.length; ++d) if (!at.includes(d)) dropped.push(d); // single-item dimensions
      axis = Int32Array.from([...Array.from(levels.axis, (v) => (v < 0 ? -1 : at[v])), ...dropped]);
      lists = [...levels.lists.map((list, l) => (levels.axis[l] < 0 ? list : Int32Array.from(list, (j) => (j < 0 ? -1 : p.sel[at[levels.axis[l]]][j])))),
        ...dropped.map((d) => p.sel[d])];
      native = p.source;
      lens = p.oldLen;
    } else {
      native = this._native;
    }
    const total = onShards(native, 'selectTotal', [lens, axis, lists, pathOut]);
    HipStore.lastSelectPath = pathOut[0] ? 'device' : 'sequential';
    return total;
  }

  /**
   * copyMeasureData (src/cube.js:859-888): this.setValue(pos, source.getValue(pos)) over a selection of distinct cells
   * (./selection.js copyLevels), in nesting order, in one launch.  The target never leaves its devices: a sharded
   * source is gathered for a target on one device, a source on one device is spread like a sharded target.  Returns
   * false when the stores cannot meet that way (partitioned differently): the caller copies cell by cell.
   */
  copySelect(source, lengths, levels) {
    const target = this._writable;
    const from = source._native;
    if (!target.isSharded) {
      target.copySelect(from.isSharded ? from.gather() : from, lengths, levels.axis, levels.lists);
      HipStore.lastCopyPath = 'device';
      return true;
    }
    const spread = from.isSharded ? from : backend.load().shardStore(from, lengths);
    try {
      target.copySelect(spread, lengths, levels.axis, levels.lists);
    } catch (e) {
      if (!/^sharded:/.test(e.message)) throw e;
      return false;
    }
    HipStore.lastCopyPath = 'device';
    return true;
  }

  /**
   * getTotalForDimensionItems of a computed measure: `program` (formula.js compile(), no SCALAR) over the stores
   * `inputs`, evaluated at every combination of the levels on the device, added as selectTotal adds (same certificate,
   * same sequential fallback, same lastSelectPath).  Pending inputs are materialised and sharded ones gathered.
   */
  static selectTotalFormula(program, inputs, lengths, levels) {
    const pathOut = new Int32Array(1);
    const natives = inputs.map((store) => store._whole);
    const total = backend.load().selectTotalFormula(program.code, program.consts, natives, lengths, levels.axis, levels.lists, pathOut);
    HipStore.lastSelectPath = pathOut[0] ? 'device' : 'sequential';
    return total;
  }

  /**
   * getNestedObject(computed measure, withTotals): `program` (formula.js compile(), no SCALAR) over the extended cubes
   * of the stores `inputs`, each built with its own rules (`rulesPerInput[i][d]`, names; an unknown one throws
   * 'Unsupported aggregation method: <m>' as the chain of drillUps does).  Returns the Float64Array of the formula's
   * extended cube.  Pending inputs are materialised and sharded ones gathered, as totals() does.
   */
  static totalsFormula(program, inputs, dimensions, rulesPerInput) {
    const addon = backend.load();
    const nd = dimensions.length;
    const codes = new Int32Array(inputs.length * nd);
    for (let i = 0; i < inputs.length; ++i) for (let d = 0; d < nd; ++d) codes[i * nd + d] = addon.methodFromName(rulesPerInput[i][d]);
    const launchesOut = new Int32Array(1);
    const natives = inputs.map((store) => store._whole);
    const values = addon.totalsFormula(program.code, program.consts, natives, lengthsOf(dimensions), codes, launchesOut);
    HipStore.lastTotalsPath = 'device';
    HipStore.lastTotalsLaunches = launchesOut[0];
    return values;
  }

  /** Whether the loaded addon answers several measures' totals in one call (HipStore.totalsReport). */
  static canReport() {
    return typeof backend.load().totalsReport === 'function';
  }

  /**
   * getNestedObjects(ids, withTotals): the extended cubes of several measures of one cube in ONE device call
   * (olap_totals_report).  An entry of `outputs` is { store, rules } — a stored measure with its rule per dimension (names,
   * as totals() takes them) — or { program, stores, rulesPerInput } — a computed one, as totalsFormula() takes it.  Every
   * distinct store is built once, whatever number of outputs reads it.  Returns one Float64Array per output (views of
   * one buffer), or null when the report would not fit the device call's limits (32 outputs over 32 distinct stores, 4e9
   * float64 cells on the device): the caller asks measure by measure.
   * Pending inputs are materialised and sharded ones gathered, as totals() and totalsFormula() do.
   */
  static totalsReport(outputs, dimensions) {
    const addon = backend.load();
    const nd = dimensions.length;
    const lens = lengthsOf(dimensions);
    const stores = []; // the distinct inputs, in order of first use
    const rulesOf = [];
    const inputOf = (store, rules) => {
      let i = stores.indexOf(store);
      if (i < 0) {
        i = stores.push(store) - 1;
        rulesOf.push(rules);
      }
      return i;
    };
    const n = outputs.length;
    const outStored = new Int32Array(n).fill(-1);
    const nCode = new Int32Array(n);
    const nConsts = new Int32Array(n);
    const nInputs = new Int32Array(n);
    const code = [];
    const consts = [];
    const picks = [];
    outputs.forEach((out, k) => {
      if (out.program === undefined) {
        outStored[k] = inputOf(out.store, out.rules);
        return;
      }
      nCode[k] = out.program.code.length;
      nConsts[k] = out.program.consts.length;
      nInputs[k] = out.stores.length;
      for (const word of out.program.code) code.push(word);
      for (const c of out.program.consts) consts.push(c);
      out.stores.forEach((store, j) => picks.push(inputOf(store, out.rulesPerInput[j])));
    });
    const codes = new Int32Array(stores.length * nd);
    for (let i = 0; i < stores.length; ++i) for (let d = 0; d < nd; ++d) codes[i * nd + d] = addon.methodFromName(rulesOf[i][d]); // throws 'Unsupported aggregation method: <m>'
    let ext = 1;
    for (let d = 0; d < nd; ++d) ext *= lens[d] + 1;
    const exported = new Set(outStored.filter((i) => i >= 0)).size;
    if (n > 32 || stores.length > 32 || (stores.length - exported + n) * ext > 4.0e9) return null; // OLAP_REPORT_MAX_OUTPUTS / _INPUTS, the cell limit
    const launchesOut = new Int32Array(1);
    const natives = stores.map((store) => store._whole);
    const values = addon.totalsReport(natives, lens, codes, outStored, nCode, Int32Array.from(code), nConsts, Float64Array.from(consts), nInputs,
      Int32Array.from(picks), launchesOut);
    HipStore.lastTotalsLaunches = launchesOut[0];
    if (picks.length > 0) HipStore.lastTotalsPath = 'device';
    return outputs.map((_, k) => values.subarray(k * ext, (k + 1) * ext));
  }

  /**
   * copyMeasureData from a computed measure: this.setValue(pos, formula(pos)) over a selection of distinct cells
   * (./selection.js copyLevels) in one launch.  This store may be one of `inputs`.  Returns false for a sharded
   * target: the caller copies cell by cell.
   */
  copySelectFormula(program, inputs, lengths, levels) {
    if (this._native.isSharded) return false;
    const target = this._writable; // (before the inputs: a target that is one of them is read where it is written)
    const natives = inputs.map((store) => store._whole);
    target.copySelectFormula(program.code, program.consts, natives, lengths, levels.axis, levels.lists);
    HipStore.lastCopyPath = 'device';
    return true;
  }

  /**
   * this.data = the formula over `inputs`, cell by cell, as ONE device call (olap_store_set_formula): `program` (formula.js
   * compile()) reads the stores `inputs` and the numbers `totals` (its SCALAR operands).  The cells, the mask and the key
   * order end as `this.data = <the formula's plain Array>` leaves them; nothing crosses to the host.  Pending dices among
   * the inputs are materialised; an input is gathered only when this store is on one device and that input is not.
   * Returns false when this store is sharded and the inputs are not partitioned like it: the caller goes through the host.
   */
  setFormula(program, inputs, totals) {
    const target = this._writable;
    const scalars = Float64Array.from(totals);
    if (target.isSharded) {
      const natives = inputs.map((store) => store._native);
      if (!natives.every((native) => native.isSharded)) return false;
      try {
        target.setFormula(program.code, program.consts, natives, scalars);
      } catch (e) {
        if (!/^sharded:/.test(e.message)) throw e;
        return false;
      }
    } else {
      target.setFormula(program.code, program.consts, inputs.map((store) => store._whole), scalars);
    }
    HipStore.lastMaterializePath = 'device';
    return true;
  }

  /** in-memory.js:178-211 */
  reorder(oldDimensions, newDimensions) {
    return this._wrap(onShards(this._native, 'reorder', [lengthsOf(oldDimensions), reorderPerm(oldDimensions, newDimensions)]));
  }

  /**
   * reorder of the stored measures of one cube — what Cube.reorderDimensions asks of every stored measure in turn.
   * Measures held whole on one device and untracked go to the device TOGETHER (addon reorderMulti ->
   * olap_store_reorder_multi: one launch for up to 8 measures of one cell type and default, except where the reorder
   * runs as the two-axis transpose); tracked and sharded measures take reorder one by one.  Pending selections are diced
   * together first (materializeMany, whose launches HipStore.lastBatchLaunches keeps reporting; the reorder's own go to
   * HipStore.lastReorderLaunches).  Returns the new stores in the order given.
   */
  static reorderMany(stores, oldDimensions, newDimensions) {
    const out = new Array(stores.length);
    HipStore.materializeMany(stores);
    HipStore.lastReorderLaunches = null;
    const addon = backend.load();
    // (an addon built before reorderMulti existed keeps the single-store calls)
    return togetherThenSingly(stores, out, () => typeof addon.reorderMulti === 'function', (natives) => {
      const launchesOut = new Int32Array(1);
      const made = addon.reorderMulti(natives, lengthsOf(oldDimensions), reorderPerm(oldDimensions, newDimensions), launchesOut);
      HipStore.lastReorderLaunches = launchesOut[0];
      return made;
    }, (store) => store.reorder(oldDimensions, newDimensions));
  }

  /**
   * Running aggregates along dimension `index` of the stored measures of one cube, each by its own rule — Cube.cumulate:
   * the cell at item k holds what dice(items of k's group under `attribute` at positions <= k) -> drillUp(rule) holds in
   * its single item.  Measures held whole on one device, untracked and with cells of their declared type go to the
   * device in ONE call (addon cumulateMulti -> olap_store_cumulate_multi: one launch for up to 8 measures of one cell
   * type and default, whatever their rules; DESIGN.md §3 K13) — a single such measure too.  Pending selections are
   * diced together first (materializeMany).  Returns the new stores in the order given, with null for a measure the
   * call does not take (order-tracking, sharded, cells of another type, an addon without the call): the caller goes
   * item by item.  Sets HipStore.lastBatchLaunches and HipStore.lastCumulatePath ('device' when the call ran).
   */
  static cumulateMany(stores, dimensions, index, attribute, methods) {
    return alongMany(stores, dimensions, index, attribute, methods, 'cumulateMulti', 'lastCumulatePath',
      (addon, natives, codes, lens, groups, nGroups, launchesOut) => addon.cumulateMulti(natives, codes, lens, index, groups, nGroups, launchesOut));
  }

  /**
   * Rolling-window aggregates along dimension `index` of the stored measures of one cube, each by its own rule —
   * Cube.rolling: the cell at item k holds what dice(items of k's group under `attribute` in [k - before, k + after])
   * -> drillUp(rule) holds in its single item, and is unset where no item is left.  Eligibility, materializeMany, the
   * ONE call (addon rollingMulti -> olap_store_rolling_multi; DESIGN.md §3 K14) and the nulls are cumulateMany's.
   * Sets HipStore.lastBatchLaunches and HipStore.lastRollingPath ('device' when the call ran).
   */
  static rollingMany(stores, dimensions, index, before, after, attribute, methods) {
    return alongMany(stores, dimensions, index, attribute, methods, 'rollingMulti', 'lastRollingPath',
      (addon, natives, codes, lens, groups, nGroups, launchesOut) => addon.rollingMulti(natives, codes, lens, index, before, after, groups, nGroups, launchesOut));
  }

  /**
   * The q-quantile along dimension `index` of the stored measures of one cube, group by group under `attribute` —
   * Cube.quantile: new stores over the dimensions of drillUp(dimension, attribute) whose cell holds the quantile (linear
   * interpolation between the two neighbouring order statistics; Cube._quantileHost is the definition) of the SET cells
   * of its group.  A measure's rule is not consulted and its insertion order does not matter, so measures held whole on
   * one device — tracked or not — with cells of their declared type's cell type (an integer measure in Float64 cells
   * keeps a median of 1.5) go to the device in ONE call (addon quantileMulti -> olap_store_quantile_multi: one launch
   * for up to 8 measures of one cell type and default; DESIGN.md §3 K15).  Pending selections are diced together first
   * (materializeMany).  Returns the new stores in the order given, with null for a measure the call does not take
   * (sharded, a store of another class, an addon without the call): the caller takes the host path.  Sets
   * HipStore.lastBatchLaunches and HipStore.lastQuantilePath ('device' when the call ran).
   */
  static quantileMany(stores, dimensions, index, attribute, q) {
    return groupedMany(stores, dimensions, index, attribute, 'quantileMulti', 'lastQuantilePath',
      (addon, natives, lens, groups, nGroups, launchesOut) => addon.quantileMulti(natives, lens, index, q, groups, nGroups, launchesOut));
  }

  /**
   * The variance (kind 0) or standard deviation (kind 1) along dimension `index` of the stored measures of one cube,
   * group by group under `attribute` — Cube.variance / Cube.stddev: new stores over the dimensions of
   * drillUp(dimension, attribute) whose cell holds the two-pass variance, divided by n - ddof, of the SET cells of its
   * group in item order (Cube._varianceHost is the definition).  A measure's rule is not consulted and its insertion
   * order does not matter, so measures held whole on one device — tracked or not — with cells of their declared type's
   * cell type go to the device in ONE call (addon varianceMulti -> olap_store_variance_multi: one launch for up to 8
   * measures of one cell type and default; DESIGN.md §3 K16).  Pending selections are diced together first
   * (materializeMany).  Returns the new stores in the order given, with null for a measure the call does not take
   * (sharded, a store of another class, an addon without the call): the caller takes the host path.  Sets
   * HipStore.lastBatchLaunches and HipStore.lastVariancePath ('device' when the call ran).
   */
  static varianceMany(stores, dimensions, index, attribute, kind, ddof) {
    return groupedMany(stores, dimensions, index, attribute, 'varianceMulti', 'lastVariancePath',
      (addon, natives, lens, groups, nGroups, launchesOut) => addon.varianceMulti(natives, lens, index, kind, ddof, groups, nGroups, launchesOut));
  }

  /** in-memory.js:139-176 — mutates this store */
  load(otherStore, myDimensions, hisDimensions) {
    this._loadWith(otherStore, lengthsOf(myDimensions), lengthsOf(hisDimensions), loadTables(myDimensions, hisDimensions));
  }

  /** load by ready-made tables (loadTables).  HipStore.lastLoadPath says where the cells travelled. */
  _loadWith(otherStore, myLen, hisLen, hisToMine) {
    // hydration scatters cells across the whole index space: a sharded measure is gathered for it and
    // stays on one device afterwards
    if (this._native.isSharded) this._nativeStore = this._native.gather();
    const target = this._writable;
    HipStore.lastLoadPath = 'device';
    if (otherStore._cells !== this._cells) {
      if (!target.orderTracked) {
        // cells of another element type are converted as they are loaded (addon loadMulti -> olap_store_load_multi)
        const launchesOut = new Int32Array(1);
        backend.load().loadMulti([target], [otherStore._whole], myLen, hisLen, hisToMine, launchesOut);
        HipStore.lastBatchLaunches = launchesOut[0];
        return;
      }
      // A tracked target of another cell type keeps the host path: its key order needs the single-store call, which
      // copies cells of one element type, so the source is re-typed through float64 first.
      const retyped = new HipStore(otherStore._size, this._type, otherStore._defaultValue);
      retyped.data = otherStore.data;
      otherStore = retyped;
      HipStore.lastLoadPath = 'host';
    }
    target.load(otherStore._whole, myLen, hisLen, hisToMine);
  }

  /**
   * targets[i].load(sources[i]) for the measures two cubes share — what Cube.hydrateFromCube asks of every stored measure
   * in turn.  The tables are computed once; pending selections among the sources are diced together (materializeMany),
   * sharded sources are gathered as load does; targets held whole on one device and untracked go to the device in ONE
   * call (addon loadMulti -> olap_store_load_multi: one launch for up to 8 pairs that share both cell types and both
   * defaults, cells of another type converted on the way); sharded and tracked targets take load one by one.
   */
  static loadMany(targets, sources, myDimensions, hisDimensions) {
    const hisToMine = loadTables(myDimensions, hisDimensions);
    const myLen = lengthsOf(myDimensions);
    const hisLen = lengthsOf(hisDimensions);
    HipStore.materializeMany(sources);
    let launches = HipStore.lastBatchLaunches;
    let path = 'device';
    // a store on both sides, or a target twice: the order of the loads matters, so they stay one by one
    const distinct = new Set(targets.concat(sources)).size === targets.length + sources.length;
    const together = [];
    targets.forEach((target, i) => {
      if (distinct && wholeUntracked(target._native)) together.push(i);
    });
    if (together.length >= 1) {
      const launchesOut = new Int32Array(1);
      backend.load().loadMulti(together.map((i) => targets[i]._writable), together.map((i) => sources[i]._whole), myLen, hisLen, hisToMine, launchesOut);
      launches += launchesOut[0];
    }
    targets.forEach((target, i) => {
      if (together.includes(i)) return;
      target._loadWith(sources[i], myLen, hisLen, hisToMine);
      if (HipStore.lastLoadPath === 'host') path = 'host';
    });
    HipStore.lastBatchLaunches = launches;
    HipStore.lastLoadPath = path;
  }

  /** Whether composeMany can run: the addon has the call (one built before it existed keeps create + fill + load). */
  static composesMany() {
    return typeof backend.load().composeMulti === 'function';
  }

  /** Whether `store` may be a source of composeMany: held whole on one device, untracked, cells of its declared type. */
  static composable(store) {
    if (!(store instanceof HipStore) || store._cells !== cellTypeOf(store._type)) return false;
    return wholeUntracked(sourceStore(store) || store._native); // (cells still on the host are uploaded)
  }

  /**
   * The stored measures of ONE source cube on the dimensions of a composed cube — what Cube.compose asked of every
   * measure in turn as createStoredMeasure + fillData + hydrateFromCube: new stores over `myDimensions` of the sources'
   * declared type and default that end, values and mask, as `new HipStore; fill(fills[i]); load(sources[i])` leaves them,
   * in ONE device call (addon composeMulti -> olap_store_compose_multi: a gather that writes every cell of the new
   * stores once, one launch for up to 8 measures of one cell type and default; DESIGN.md §3 K12).  `fills[i]` undefined
   * or null: no fill.  The tables are loadTables'; pending selections among the sources are diced together first
   * (materializeMany).  Every source must be composable().  Sets HipStore.lastBatchLaunches, counts in lastComposeCalls.
   */
  static composeMany(sources, myDimensions, hisDimensions, fills = []) {
    const hisToMine = loadTables(myDimensions, hisDimensions);
    HipStore.materializeMany(sources);
    let launches = HipStore.lastBatchLaunches;
    const values = new Float64Array(sources.length);
    const hasFill = new Uint8Array(sources.length);
    sources.forEach((_, i) => {
      if (fills[i] === undefined || fills[i] === null) return;
      values[i] = fills[i];
      hasFill[i] = 1;
    });
    const launchesOut = new Int32Array(1);
    const natives = backend.load().composeMulti(sources.map((store) => store._whole), lengthsOf(myDimensions), lengthsOf(hisDimensions), hisToMine, values, hasFill, launchesOut);
    launches += launchesOut[0];
    HipStore.lastComposeCalls += 1;
    HipStore.lastBatchLaunches = launches;
    return sources.map((store, i) => store._wrap(natives[i]));
  }

  /**
   * What every combination of the scanned dimensions' items receives, for the stored measures of one cube, in ONE device
   * call (addon blocksReport -> olap_store_blocks_report): `scannedFlags[d]` marks the scanned dimensions.  Returns one
   * Float64Array per store — views of the one result, laid out [combination][kept cells], the default in unset cells — or
   * null when the call does not apply: a sharded or tracked measure, an addon without the call, or a result above the
   * call's byte cap (OLAP_BLOCKS_MAX_BYTES).  The caller then goes combination by combination.  Pending dices are
   * materialised together first, as reorderMany does.  Sets HipStore.lastBlocksCalls and HipStore.lastBatchLaunches.
   */
  static blocksMany(stores, dimensions, scannedFlags) {
    const addon = backend.load();
    if (typeof addon.blocksReport !== 'function') return null;
    if (stores.some((store) => sourceStore(store) && !wholeUntracked(sourceStore(store)))) return null;
    HipStore.materializeMany(stores);
    let launches = HipStore.lastBatchLaunches;
    const natives = stores.map((store) => store._native);
    if (!natives.every(wholeUntracked)) return null;
    const lens = lengthsOf(dimensions);
    const size = lens.reduce((n, l) => n * l, 1);
    if (stores.length * size * 8 > HipStore.blocksMaxBytes) return null;
    const launchesOut = new Int32Array(1);
    let values;
    try {
      values = addon.blocksReport(natives, lens, Uint8Array.from(scannedFlags, (f) => (f ? 1 : 0)), launchesOut);
    } catch (e) {
      if (!/^blocks:/.test(e.message)) throw e;
      return null; // the cap (lowered by the environment)
    }
    launches += launchesOut[0];
    HipStore.lastBlocksCalls += 1;
    HipStore.lastBatchLaunches = launches;
    return stores.map((_, k) => values.subarray(k * size, (k + 1) * size));
  }

  /**
   * Same blob as the reference (in-memory.js:75-101): the set cells in sparse form.  The compaction
   * (set cells -> ascending index / value lists) runs on the device.
   */
  serialize() {
    const sparse = this._whole.toSparse();
    // `new Int32Array(map.values())` (in-memory.js:77-92): the coercion to the declared type happens here
    const values = sparse.values.constructor === TYPED_ARRAY[this._type] ? sparse.values : TYPED_ARRAY[this._type].from(sparse.values);
    return toBuffer({ size: this._size, type: this._type, defaultValue: this._defaultValue, indexes: sparse.indexes, dataBuffer: values });
  }

  /** in-memory.js:103-116; accepts blobs written by the reference. */
  static deserialize(buffer) {
    const data = fromBuffer(buffer);
    const type = data.type;
    if (!Object.prototype.hasOwnProperty.call(TYPE_CODE, type)) throw new Error('Invalid type');
    const defaultValue = Number.isNaN(data.defaultValue) ? Number.NaN : 0;
    const cells = cellTypeOf(type);
    const TA = TYPED_ARRAY[cells];
    const values = data.dataBuffer instanceof TA ? data.dataBuffer : TA.from(data.dataBuffer);
    const native = backend.load().storeFromSparse(data.size, TYPE_CODE[cells], Number.isNaN(defaultValue) ? 1 : 0, data.indexes instanceof Uint32Array ? data.indexes : new Uint32Array(data.indexes), values);
    return new HipStore(data.size, type, defaultValue, native);
  }
}

HipStore.lastSelectPath = null;
// the blocksReport calls the last Cube.scan / iterateOverDimension made: 1 when every combination was served from one device
// pass, 0 when it went combination by combination; Cube resets it when such a call starts
HipStore.lastBlocksCalls = 0;
// OLAP_BLOCKS_MAX_BYTES (include/olap_hip.h): the float64 result one blocksReport call may bring back
HipStore.blocksMaxBytes = 2 ** 30;
// Cube.scan / iterateOverDimension go combination by combination when one combination receives more cells than this: at 10^6
// cells per combination the one pass measured 0.9 - 1.2 of the loop's time while holding every block on the host at once, at
// 10^5 it is 1.2 - 1.5 times faster (profiles/scan_blocks_r36.txt; nothing was measured in between)
HipStore.blocksMaxBlockCells = 500000;
// kernel launches the device reported for the last many-call (diceMany: 0 where every selection stays pending; materializeMany,
// drillDownMany and the pending selections of drillUpMany: what diceMulti / drillDownMulti / diceDrillUpMulti launched;
// loadMany and a load between cell types: what loadMulti launched on top)
HipStore.lastBatchLaunches = null;
// the composeMulti calls the last Cube.compose made: one per source cube that had a measure for it, 0 when every measure
// took create + fill + load; Cube resets it when compose starts
HipStore.lastComposeCalls = 0;
// what the last Cube.cumulate did: 'device' when at least one measure left through cumulateMulti, 'per-item' when every
// measure took the dice -> drillUp chain item by item (Cube._cumulatePerItem)
HipStore.lastCumulatePath = null;
// the same for the last Cube.rolling / Cube.shift (rollingMulti, Cube._rollingPerItem)
HipStore.lastRollingPath = null;
// what the last Cube.quantile / Cube.median did: 'device' when at least one measure left through quantileMulti, 'host' when every
// measure was selected on the host (Cube._quantileHost)
HipStore.lastQuantilePath = null;
// what the last Cube.variance / Cube.stddev did: 'device' when at least one measure left through varianceMulti, 'host' when every
// measure was folded on the host (Cube._varianceHost)
HipStore.lastVariancePath = null;

/**
 * The groups of dimension `index` under `attribute` as the many-calls along a dimension take them: groups[k] is the
 * group of item k (null under 'all': one group), nGroups how many there are.
 */
function groupsOf(dimensions, index, attribute) {
  const groups = attribute === 'all' ? null : asU32(dimensions[index].getGroupIndexFromRootIndexMap(attribute));
  return { groups, nGroups: groups === null ? 1 : groups.reduce((n, g) => Math.max(n, g + 1), 0) };
}

/**
 * What the calls along a dimension that take a rule per measure share — cumulateMany and rollingMany (`call`: the
 * addon's many-call `name`): the measures held whole on one device, untracked and with cells of their declared type
 * leave in ONE call; null for the others.  pathField: the HipStore field that says what ran ('device' or 'per-item').
 */
function alongMany(stores, dimensions, index, attribute, methods, name, pathField, call) {
  const out = new Array(stores.length).fill(null);
  const addon = backend.load();
  HipStore[pathField] = 'per-item';
  if (typeof addon[name] !== 'function') return out;
  HipStore.materializeMany(stores);
  let launches = HipStore.lastBatchLaunches;
  // (a selection alone in its group stays pending there: it is diced now, as the first read of its cells would)
  for (const store of stores) {
    if (store._pending && wholeUntracked(store._pending.source)) store._materialize();
  }
  const { groups, nGroups } = groupsOf(dimensions, index, attribute);
  const eligible = (i) => stores[i]._cells === cellTypeOf(stores[i]._type);
  const run = (natives, together) => {
    const codes = Int32Array.from(together, (i) => addon.methodFromName(methods[i] === undefined ? 'sum' : methods[i])); // throws 'Unsupported aggregation method: <m>'
    const launchesOut = new Int32Array(1);
    const made = call(addon, natives, codes, lengthsOf(dimensions), groups, nGroups, launchesOut);
    launches += launchesOut[0];
    HipStore[pathField] = 'device';
    return made;
  };
  // (togetherThenSingly sends two or more together; a measure alone among the eligible ones is a batch of one)
  togetherThenSingly(stores, out, eligible, run, (store, i) => (wholeUntracked(heldStore(store)) && eligible(i) ? store._wrap(run([store._nativeStore], [i])[0]) : null));
  HipStore.lastBatchLaunches = launches;
  return out;
}

/**
 * What the calls along a dimension that roll its groups up without a rule share — quantileMany and varianceMany
 * (`call`: the addon's many-call `name`): the measures held whole on one device, tracked or not, with cells of their
 * declared type leave in ONE call; null for the others.  pathField: the HipStore field that says what ran ('device' or
 * 'host').
 */
function groupedMany(stores, dimensions, index, attribute, name, pathField, call) {
  const out = new Array(stores.length).fill(null);
  const addon = backend.load();
  HipStore[pathField] = 'host';
  if (typeof addon[name] !== 'function') return out;
  const mine = stores.filter((store) => store instanceof HipStore);
  HipStore.materializeMany(mine);
  let launches = HipStore.lastBatchLaunches;
  const whole = (native) => !!native && !native.isSharded;
  // (a selection alone in its group stays pending there, host-resident cells have no device store yet: both get one now)
  for (const store of mine) {
    if (store._pending ? whole(store._pending.source) : !store._nativeStore) store._materialize();
  }
  const together = [];
  stores.forEach((store, i) => {
    if (store instanceof HipStore && whole(heldStore(store)) && store._cells === cellTypeOf(store._type)) together.push(i);
  });
  if (together.length > 0) {
    const { groups, nGroups } = groupsOf(dimensions, index, attribute);
    const launchesOut = new Int32Array(1);
    const made = call(addon, together.map((i) => stores[i]._nativeStore), lengthsOf(dimensions), groups, nGroups, launchesOut);
    together.forEach((i, j) => {
      out[i] = stores[i]._wrap(made[j]);
    });
    launches += launchesOut[0];
    HipStore[pathField] = 'device';
  }
  HipStore.lastBatchLaunches = launches;
  return out;
}
// kernel launches reorderMulti reported for the last reorderMany (null: every measure took reorder one by one)
HipStore.lastReorderLaunches = null;
// 'device' after a getNestedObject(computed measure, withTotals) that ran as one olap_formula_totals call, and the
// launches it reported; never reset here
HipStore.lastTotalsPath = null;
HipStore.lastTotalsLaunches = null;
// the device calls the last Cube.getNestedObjects(ids, withTotals) made for the ids that did not take the chain of
// drillUps: 1 when they left in one report (HipStore.totalsReport), one per measure otherwise; written by Cube
HipStore.lastTotalsCalls = null;
// 'device' after a copyMeasureData that ran as one device scatter (copySelect / copySelectFormula); never reset here
HipStore.lastCopyPath = null;

// 'device' after a load / loadMany whose cells stayed on the device, 'host' when a source of another cell type went
// through the host as float64 (a tracked target); never reset here
HipStore.lastLoadPath = null;

// what the last Cube.copyToStoredMeasure / convertToStoredMeasure did: 'device' (setFormula: one device call, no host copy)
// or 'host' (getData, then setData); Cube resets it to null when such a call starts
HipStore.lastMaterializePath = null;

module.exports = HipStore;
module.exports.toPlainArray = toPlainArray;
module.exports._internals = { visibleDims, effectiveSelection, diceTables, pendingGroups }; // host-side logic, unit-tested without a device
