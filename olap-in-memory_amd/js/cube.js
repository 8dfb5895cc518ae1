'use strict';
/*
 * Cube — same public surface as the reference's Cube for the aggregation path
 * (/root/reference/src/cube.js, src/index.d.ts:37-148), with every stored measure held in a
 * HipStore (MI355X HBM).  The class is host-side orchestration only: a query rebuilds ONE
 * dimension, then asks each measure's store for the matching bulk operation with the rule
 * `storedMeasuresRules[measure][dimensionId]` (src/cube.js:1012-1020).
 *
 * Kept from the reference because callers rely on it (SURVEY.md §8(a7), §8(b)):
 *   - queries never mutate; a no-op returns the SAME cube object (src/cube.js:997, :843, :818, :968);
 *   - derived cubes share `computedMeasures` and the rules object by reference, except
 *     addDimension / removeDimension which deep-copy the rules (:931, :957);
 *   - removeDimension = drillUp(id, 'all') with the dimension dropped from the list (:950-964);
 *   - slice = dice + removeDimension (:799-807); collapse = slice every dimension to 'all' (:320-324).
 * Computed measures use ./formula.js (own parser for the arithmetic subset of expr-eval the
 * reference enables) and are evaluated by one element-wise device launch; (de)serialisation uses
 * the reference's container (./wire.js).
 */
const HipStore = require('./store/hip');
const CatchAllDimension = require('./dimension/catch-all');
const TimeSlot = require('./calendar');
const { toNestedArray, fromNestedArray, toNestedObject, fromNestedObject } = require('./formatter');
const { toBuffer, fromBuffer, toArrayBuffer } = require('./wire');
const { getParser, isDeviceExact } = require('./formula');
const backend = require('./backend');
const { selectionLevels, copyLevels } = require('./selection');

const MEASURE_ID = /^[a-z][_a-z0-9]+$|^[_a-z0-9]+__total$/i;

const deepCopy = (value) => (value === undefined ? undefined : JSON.parse(JSON.stringify(value)));

function deepMerge(target, source) {
  if (source === null || typeof source !== 'object') return source;
  const out = target !== null && typeof target === 'object' ? target : {};
  for (const key of Object.keys(source)) out[key] = deepMerge(out[key], source[key]);
  return out;
}

function cartesian(options) {
  const keys = Object.keys(options);
  let rows = [{}];
  for (const key of keys) {
    const next = [];
    for (const row of rows) for (const item of options[key]) next.push(Object.assign({}, row, { [key]: item }));
    rows = next;
  }
  return rows;
}

class Cube {
  constructor(dimensions) {
    this.dimensions = dimensions;
    this.storedMeasures = {};
    this.storedMeasuresRules = {};
    this.computedMeasures = {};
  }

  // ------------------------------------------------------------------ introspection
  get storeSize() {
    return this.dimensions.reduce((n, d) => n * d.numItems, 1);
  }

  get byteLength() {
    return Object.values(this.storedMeasures).reduce((n, store) => n + store.byteLength, 0);
  }

  get dimensionIds() {
    return this.dimensions.map((d) => d.id);
  }

  get storedMeasureIds() {
    return Object.keys(this.storedMeasures);
  }

  get computedMeasureIds() {
    return Object.keys(this.computedMeasures);
  }

  getDimension(dimensionId) {
    return this.dimensions.find((d) => d.id === dimensionId);
  }

  getDimensionIndex(dimensionId) {
    return this.dimensions.findIndex((d) => d.id === dimensionId);
  }

  // ------------------------------------------------------------------ measures
  _checkNewMeasure(measureId) {
    if (!MEASURE_ID.test(measureId)) throw new Error(`Invalid measureId: ${measureId}`);
    if (this.storedMeasures[measureId] !== undefined) throw new Error(`This measure already exists: ${measureId}`);
  }

  createStoredMeasure(measureId, rules = {}, type = 'float32', defaultValue = 0) {
    this._checkNewMeasure(measureId);
    this.storedMeasures[measureId] = this._newStore(type, defaultValue, rules);
    this.storedMeasuresRules[measureId] = rules;
  }

  /**
   * A measure's store.  `first` / `last` follow the Map's INSERTION order in the reference (in-memory.js:298): a measure
   * with such a rule keeps that order (HipStore.trackOrder) and therefore stays on ONE device even when a device list
   * is set — the shards of a split measure combine in row order, which is the reference's order only for a cube
   * filled in ascending index order — so that the same program answers the same with and without setDevices().
   */
  _newStore(type, defaultValue, rules) {
    const ordered = Object.values(rules || {}).some((rule) => rule === 'first' || rule === 'last');
    const store = new HipStore(this.storeSize, type, defaultValue, undefined, ordered ? undefined : this.dimensions.map((d) => d.numItems));
    if (ordered) store.trackOrder();
    return store;
  }

  /**
   * A measure defined by a formula over stored measures (and `<measure>__total`), evaluated per
   * cell on demand (src/cube.js:97-140).  Formulas naming other computed measures are inlined.
   */
  createComputedMeasure(measureId, formula) {
    if (!MEASURE_ID.test(measureId)) throw new Error(`Invalid measureId: ${measureId}`);
    if (this.storedMeasures[measureId] !== undefined || this.computedMeasures[measureId] !== undefined) throw new Error(`This measure already exists ${measureId}`);
    let text = formula;
    for (const id of this.computedMeasureIds) {
      const whole = new RegExp(`\\b${id}\\b`, 'g');
      if (text.match(whole)) text = text.replace(whole, `(${this.computedMeasures[id].toString()})`);
    }
    const expression = getParser().parse(text);
    const known = this.storedMeasureIds.concat(this.storedMeasureIds.map((m) => `${m}__total`));
    const variables = expression.variables({ withMembers: true });
    if (!variables.every((v) => known.includes(v))) throw new Error(`Unknown measure(s): ${variables.filter((v) => !this.storedMeasureIds.includes(v))}`);
    this.computedMeasures[measureId] = expression;
  }

  /**
   * src/cube.js:205-233.  A source that reads stored measures is written into the new measure by one device call
   * (_materializeOnDevice); anything else takes the host path, with its messages and the state it leaves when it throws.
   */
  copyToStoredMeasure(computedMeasureId, storedMeasureId, rules = {}, type = 'float32', defaultValue = 0) {
    HipStore.lastMaterializePath = null;
    if (this._materializeOnDevice(computedMeasureId, storedMeasureId, rules, type, defaultValue, false)) return;
    this._copyToStoredMeasureHost(computedMeasureId, storedMeasureId, rules, type, defaultValue, false);
  }

  convertToStoredMeasure(measureId, rules = {}, type = 'float32', defaultValue = 0) {
    HipStore.lastMaterializePath = null;
    if (this.computedMeasures[measureId] && this._materializeOnDevice(measureId, measureId, rules, type, defaultValue, true)) return;
    this._copyToStoredMeasureHost(measureId, measureId, rules, type, defaultValue, true);
  }

  /** Both methods through the host: a plain Array of every cell down, a Float64Array of every cell up. */
  _copyToStoredMeasureHost(computedMeasureId, storedMeasureId, rules, type, defaultValue, convert) {
    HipStore.lastMaterializePath = 'host';
    if (convert && !this.computedMeasures[computedMeasureId]) throw new Error(`convertToStoredMeasure: no such computed measure: ${computedMeasureId}`);
    const data = this.getData(computedMeasureId);
    if (convert) this.dropMeasure(computedMeasureId);
    this.createStoredMeasure(storedMeasureId, rules, type, defaultValue);
    this.setData(storedMeasureId, data);
  }

  /**
   * What getData(sourceId) evaluates, as a device program: { program, stores, totals } for a stored measure (`INPUT 0`) and
   * for a computed one that reads at least one stored measure; null otherwise.
   */
  _materializeSource(sourceId) {
    const stored = this.storedMeasures[sourceId];
    if (stored !== undefined) return { program: { code: Int32Array.of(1, 0), consts: new Float64Array(0) }, stores: [stored], totals: [] };
    const expression = this.computedMeasures[sourceId];
    if (expression === undefined) return null;
    const inputs = {};
    const scalars = {};
    const stores = [];
    const totals = [];
    for (const name of expression.variables({ withMembers: true })) {
      const store = this.storedMeasures[name.replace('__total', '')];
      if (store === undefined) return null;
      if (name.includes('__total')) scalars[name] = totals.push(store.total) - 1;
      else inputs[name] = stores.push(store) - 1;
    }
    if (stores.length === 0) return null;
    return { program: expression.compile(inputs, scalars), stores, totals };
  }

  /**
   * copyToStoredMeasure / convertToStoredMeasure without the host (DESIGN.md §3 K10).  The new store is filled by
   * HipStore.setFormula BEFORE the cube changes; then dropMeasure (for a conversion) and the new measure follow, in the order
   * of the host path.  Returns false with the cube untouched whenever the host path would throw somewhere (an unknown
   * source, an id that is taken or invalid, a type or default the store refuses), when the source reads no stored measure,
   * when the device call refuses the program (its limits are the C ABI's), and when a sharded target cannot read the inputs
   * in place: the host path then runs, with its messages.
   */
  _materializeOnDevice(sourceId, targetId, rules, type, defaultValue, convert) {
    if (!MEASURE_ID.test(targetId) || (this.storedMeasures[targetId] !== undefined)) return false;
    if (!['int32', 'uint32', 'float32', 'float64'].includes(type) || !(Number.isNaN(defaultValue) || defaultValue === 0)) return false;
    const source = this._materializeSource(sourceId);
    if (source === null) return false;
    const ordered = Object.values(rules || {}).some((rule) => rule === 'first' || rule === 'last');
    // a target split over several devices reads inputs that are split too (no store is created for the others)
    if (!ordered && HipStore.splits(this.dimensions.map((d) => d.numItems)) && !source.stores.every((store) => store._native.isSharded)) return false;
    const store = this._newStore(type, defaultValue, rules);
    try {
      if (!store.setFormula(source.program, source.stores, source.totals)) return false;
    } catch (e) {
      return false; // refused (a program beyond the device call's limits): the host path says so in its own words
    }
    if (convert) this.dropMeasure(sourceId);
    this.storedMeasures[targetId] = store;
    this.storedMeasuresRules[targetId] = rules;
    return true;
  }

  replaceStoredMeasure(toKeep, toDrop) {
    for (const id of [toKeep, toDrop]) if (this.storedMeasures[id] === undefined) throw new Error(`replaceStoredMeasure: no such measure ${id}`);
    for (const id of this.computedMeasureIds) {
      const expression = this.computedMeasures[id];
      if (expression.variables().includes(toDrop)) this.computedMeasures[id] = expression.substitute(toDrop, toKeep);
    }
    this.dropMeasure(toDrop);
  }

  /** One device launch evaluates the formula for every cell (olap_eval_formula). */
  _evaluateComputed(measureId) {
    const expression = this.computedMeasures[measureId];
    const inputs = {};
    const scalars = {};
    const stores = [];
    const totals = [];
    for (const name of expression.variables({ withMembers: true })) {
      if (name.includes('__total')) {
        scalars[name] = totals.push(this.storedMeasures[name.replace('__total', '')].total) - 1;
      } else {
        inputs[name] = stores.push(this.storedMeasures[name]) - 1;
      }
    }
    if (stores.length === 0) {
      // a formula of constants / totals only: nothing to stream, evaluate once on the host
      const params = {};
      Object.keys(scalars).forEach((name) => {
        params[name] = totals[scalars[name]];
      });
      return new Array(this.storeSize).fill(expression.evaluate(params));
    }
    const program = expression.compile(inputs, scalars);
    const addon = backend.load();
    const natives = stores.map((store) => store._native);
    // measures split over several devices alike: evaluated per shard; otherwise on one device (gathered if need be)
    if (natives.every((native) => native.isSharded)) {
      try {
        return HipStore.toPlainArray(addon.evalFormulaSharded(program.code, program.consts, natives, Float64Array.from(totals)));
      } catch (e) {
        if (!/^sharded:/.test(e.message)) throw e;
      }
    }
    return HipStore.toPlainArray(addon.evalFormula(program.code, program.consts, stores.map((store) => store._whole), Float64Array.from(totals)));
  }

  copyStoredMeasure(measureId, copyMeasureId) {
    if (!MEASURE_ID.test(copyMeasureId)) throw new Error(`Invalid measureId: ${copyMeasureId}`);
    if (this.storedMeasures[measureId] === undefined) throw new Error(`This measure does not exists: ${measureId}`);
    if (this.storedMeasures[copyMeasureId] !== undefined) throw new Error(`This measure already exists: ${copyMeasureId}`);
    this.storedMeasures[copyMeasureId] = this.storedMeasures[measureId].clone();
    this.storedMeasuresRules[copyMeasureId] = deepCopy(this.storedMeasuresRules[measureId]);
  }

  cloneStoredMeasure(originCube, measureId) {
    this._checkNewMeasure(measureId);
    const origin = originCube.storedMeasures[measureId];
    if (origin === undefined) throw new Error(`This measure does not exists in originCube: ${measureId}`);
    this.storedMeasuresRules[measureId] = Object.assign({}, originCube.storedMeasuresRules[measureId]);
    this.storedMeasures[measureId] = this._newStore(origin._type, origin._defaultValue, origin.orderTracked ? { any: 'first' } : this.storedMeasuresRules[measureId]);
  }

  renameMeasure(oldMeasureId, newMeasureId) {
    // eslint-disable-next-line eqeqeq
    if (oldMeasureId == newMeasureId) return;
    if (this.computedMeasures[oldMeasureId]) {
      this.computedMeasures[newMeasureId] = this.computedMeasures[oldMeasureId];
      delete this.computedMeasures[oldMeasureId];
      return;
    }
    if (!this.storedMeasures[oldMeasureId]) throw new Error(`renameMeasure: no such measure ${oldMeasureId} -> ${newMeasureId}`);
    this.storedMeasures[newMeasureId] = this.storedMeasures[oldMeasureId];
    this.storedMeasuresRules[newMeasureId] = this.storedMeasuresRules[oldMeasureId];
    delete this.storedMeasures[oldMeasureId];
    delete this.storedMeasuresRules[oldMeasureId];
    for (const id of this.computedMeasureIds) {
      const expression = this.computedMeasures[id];
      if (expression.variables().includes(oldMeasureId)) this.computedMeasures[id] = expression.substitute(oldMeasureId, newMeasureId);
    }
  }

  dropMeasure(measureId) {
    if (this.computedMeasures[measureId] !== undefined) {
      delete this.computedMeasures[measureId];
      return;
    }
    if (this.storedMeasures[measureId] === undefined) throw new Error(`dropMeasure: no such measure: ${measureId}`);
    delete this.storedMeasures[measureId];
    delete this.storedMeasuresRules[measureId];
    for (const id of this.computedMeasureIds) if (this.computedMeasures[id].variables().includes(measureId)) delete this.computedMeasures[id];
  }

  dropMeasures(measureIds) {
    measureIds.forEach((id) => this.dropMeasure(id));
  }

  keepMeasure(measureId) {
    this.keepMeasures([measureId]);
  }

  keepMeasures(measureIds) {
    this.computedMeasureIds.concat(this.storedMeasureIds).filter((id) => !measureIds.includes(id)).forEach((id) => {
      if (this.computedMeasures[id] !== undefined || this.storedMeasures[id] !== undefined) this.dropMeasure(id);
    });
  }

  updateStoredMeasureRules(measureId, cb) {
    this.storedMeasuresRules[measureId] = cb(this.storedMeasuresRules[measureId]);
  }

  clone(measures = []) {
    // dimension objects are immutable for every query, so the copy may share them
    const copy = new Cube(this.dimensions.slice());
    const wanted = (id) => measures.length === 0 || measures.includes(id);
    for (const id of this.computedMeasureIds.filter(wanted)) copy.computedMeasures[id] = this.computedMeasures[id];
    for (const id of this.storedMeasureIds.filter(wanted)) {
      copy.storedMeasures[id] = this.storedMeasures[id].clone();
      copy.storedMeasuresRules[id] = deepCopy(this.storedMeasuresRules[id]);
    }
    return copy;
  }

  // ------------------------------------------------------------------ cell access
  _store(measureId, caller) {
    const store = this.storedMeasures[measureId];
    if (store === undefined) throw new Error(`${caller}: no such measure ${measureId}`);
    return store;
  }

  getData(measureId) {
    if (this.computedMeasures[measureId] !== undefined && this.storedMeasures[measureId] === undefined) return this._evaluateComputed(measureId);
    return this._store(measureId, 'getData').data;
  }

  getStatusMap(measureId) {
    if (this.storedMeasures[measureId] !== undefined) return this.storedMeasures[measureId]._dataMap;
    if (this.computedMeasures[measureId] === undefined) throw new Error(`getStatusMap: no such measure ${measureId}`);
    // src/cube.js:373-386: the union of every stored measure's keys, values OR-ed together
    const result = new Map();
    for (const store of Object.values(this.storedMeasures))
      for (const [key, value] of store._dataMap.entries()) result.set(key, result.get(key) ? result.get(key) | value : value);
    return result;
  }

  getTotal(measureId) {
    return this.storedMeasures[measureId].total;
  }

  fillData(measureId, value) {
    if (!this.storedMeasures[measureId]) throw new Error(`fillData can only be called on stored measures: ${measureId}`);
    this.storedMeasures[measureId].fill(value);
  }

  setData(measureId, values) {
    if (!this.storedMeasures[measureId]) throw new Error(`setData can only be called on stored measures: ${measureId}`);
    this.storedMeasures[measureId].data = values;
  }

  getNestedArray(measureId) {
    return toNestedArray(this.getData(measureId), this.dimensions);
  }

  setNestedArray(measureId, values) {
    this.setData(measureId, fromNestedArray(values, this.dimensions));
  }

  /** With totals: the 2^D marginal cubes (drillUp to 'all' on every subset of dimensions) merged. */
  getNestedObject(measureId, withTotals = false) {
    return this.getNestedObjects([measureId], withTotals)[measureId];
  }

  getNestedObjects(measureIds, withTotals = false) {
    const plain = (cube, ids) => {
      const out = {};
      for (const id of ids) out[id] = toNestedObject(cube.getData(id), cube.dimensions);
      return out;
    };
    // eslint-disable-next-line eqeqeq
    if (!withTotals || this.dimensions.length == 0) return plain(this, measureIds);
    // The reference rebuilds every marginal from the full cube: 2^D chains of drillUp(dim, 'all')
    // (src/cube.js:429-437), merged into one object whose levels carry an extra 'all' key.  All 2^D
    // results are the cells of ONE extended cube with an 'all' item appended to every dimension; a stored
    // measure gets it from a single store call (olap_store_totals: one launch that reads the cube once
    // when the extended cube fits in LDS, D + 2 launches otherwise) — same chain order, same rounding.
    // (a measure that tracks its insertion order takes the chain too: every marginal has an order of its own)
    const direct = (id) => this.storedMeasures[id] !== undefined && !this.storedMeasures[id].orderTracked;
    const extended = this.dimensions.map((d) => ({ getItems: () => d.getItems().concat(['all']) }));
    const rulesOf = (id) => {
      const rules = this.storedMeasuresRules[id] || {};
      return this.dimensions.map((d) => rules[d.id]);
    };
    // A computed measure over stored measures: marginal s of input X is the sub-lattice s of X's extended cube, and
    // the measure on marginal s is the formula applied cell by cell to its inputs there — so its extended cube is the
    // formula over the inputs' extended cubes, built and evaluated on the device (olap_formula_totals).
    const eligible = []; // the ids the device answers, each once: { id, store } | { id, formula }
    const others = [];
    for (const id of measureIds) {
      if (eligible.some((e) => e.id === id) || others.includes(id)) continue;
      if (direct(id)) {
        eligible.push({ id, store: this.storedMeasures[id] });
        continue;
      }
      const formula = this._totalsFormula(id);
      if (formula === null) others.push(id);
      else eligible.push({ id, formula });
    }
    const found = {};
    // Two or more of them leave in ONE device call (olap_totals_report): every distinct stored measure's extended cube
    // is built once, all formulas are evaluated by one launch, one copy comes back.  null: too large for one call.
    let slots = null;
    if (eligible.length >= 2 && eligible.every((e) => (e.store ? [e.store] : e.formula.stores).every((store) => store instanceof HipStore)) && HipStore.canReport()) {
      slots = HipStore.totalsReport(eligible.map((e) => (e.store
        ? { store: e.store, rules: rulesOf(e.id) }
        : { program: e.formula.program, stores: e.formula.stores, rulesPerInput: e.formula.ids.map(rulesOf) })), this.dimensions);
    }
    eligible.forEach((e, k) => {
      let flat;
      if (slots !== null) flat = slots[k];
      else if (e.store) flat = e.store.totals(this.dimensions, rulesOf(e.id));
      else flat = HipStore.totalsFormula(e.formula.program, e.formula.stores, this.dimensions, e.formula.ids.map(rulesOf));
      found[e.id] = toNestedObject(flat, extended);
    });
    HipStore.lastTotalsCalls = slots !== null ? 1 : eligible.length;
    // tracked stored measures, formulas that read `<id>__total`, constants only or more than 8 measures: the chain
    const chained = others.length ? this._getNestedObjectsChain(others) : {};
    const result = {};
    for (const id of measureIds) result[id] = found[id] !== undefined ? found[id] : chained[id];
    return result;
  }

  /**
   * src/cube.js:442-465 lightly memoised: the measures are read on each of the 2^D marginal cubes (a computed measure's
   * `__total` parameters are that cube's totals) and the objects merged.  The chain of subset s is the chain of (s
   * without its highest dimension) plus one drillUp, so marginals are memoised: same order of operations, same values.
   */
  _getNestedObjectsChain(measureIds) {
    const plain = (cube, ids) => {
      const out = {};
      for (const id of ids) out[id] = toNestedObject(cube.getData(id), cube.dimensions);
      return out;
    };
    let result = {};
    const marginals = [this];
    for (let subset = 0; subset < 2 ** this.dimensions.length; ++subset) {
      if (subset > 0) {
        const top = 31 - Math.clz32(subset);
        marginals[subset] = marginals[subset & ~(1 << top)].drillUp(this.dimensions[top].id, 'all');
      }
      result = deepMerge(result, plain(marginals[subset], measureIds));
    }
    return result;
  }

  /**
   * A computed measure whose totals run on the device (DESIGN.md §3 K6): { program, stores, ids } when it is not also
   * stored, reads 1..8 stored measures of this cube and nothing else (no `<id>__total`), none of them tracking its
   * insertion order, and its program fits the device interpreter.  No isDeviceExact filter: the chain evaluates on the
   * device too, with the same interpreter.  null: the chain.
   */
  _totalsFormula(measureId) {
    const expression = this.computedMeasures[measureId];
    if (expression === undefined || this.storedMeasures[measureId] !== undefined) return null;
    const inputs = {};
    const stores = [];
    const ids = [];
    for (const name of expression.variables({ withMembers: true })) {
      const store = this.storedMeasures[name];
      if (store === undefined || store.orderTracked) return null;
      inputs[name] = stores.push(store) - 1;
      ids.push(name);
    }
    if (stores.length === 0 || stores.length > 8) return null;
    const program = expression.compile(inputs);
    if (program.code.length > 96 || program.consts.length > 24 || program.depth > 16) return null;
    return { program, stores, ids };
  }

  setNestedObject(measureId, value) {
    this.setData(measureId, fromNestedObject(value, this.dimensions));
  }

  /**
   * src/cube.js hydrateFromSparseNestedObject.  The walk is the per-cell one (same `for...in` order, same item lookups),
   * but it records each leaf and the store writes them all in one setValues call, which leaves the store exactly as the
   * per-cell setValue calls would.  A leaf that is not a number, null or undefined (setValue's coercion could throw or
   * differ), or an offset outside the store, sends the whole call down the per-cell path.  When the walk itself throws,
   * the leaves recorded so far are written first, as the per-cell path would have written them.
   */
  hydrateFromSparseNestedObject(measureId, obj, offset = 0, depth = 0) {
    const store = this.storedMeasures[measureId];
    if (store === undefined) return this._hydrateFromSparseNestedObjectPerCell(measureId, obj, offset, depth);
    const size = store.size;
    const indexes = [];
    const values = [];
    const perCell = {};
    const walk = (node, at, d) => {
      if (d === this.dimensions.length) {
        if ((typeof node !== 'number' && node !== null && node !== undefined) || !Number.isInteger(at) || at < 0 || at >= size) throw perCell;
        indexes.push(at);
        values.push(node);
        return;
      }
      const dimension = this.dimensions[d];
      for (const key in node) {
        const item = dimension.getRootIndexFromRootItem(key);
        if (item !== -1) walk(node[key], at * dimension.numItems + item, d + 1);
      }
    };
    try {
      walk(obj, offset, depth);
    } catch (e) {
      if (e === perCell) return this._hydrateFromSparseNestedObjectPerCell(measureId, obj, offset, depth);
      if (indexes.length) store.setValues(indexes, values);
      throw e;
    }
    if (indexes.length) store.setValues(indexes, values);
    return undefined;
  }

  _hydrateFromSparseNestedObjectPerCell(measureId, obj, offset = 0, depth = 0) {
    if (depth === this.dimensions.length) {
      this.storedMeasures[measureId].setValue(offset, obj);
      return;
    }
    const dimension = this.dimensions[depth];
    for (const key in obj) {
      const at = dimension.getRootIndexFromRootItem(key);
      if (at !== -1) this._hydrateFromSparseNestedObjectPerCell(measureId, obj[key], offset * dimension.numItems + at, depth + 1);
    }
  }

  getPosition(coords) {
    let position = 0;
    for (const dimension of this.dimensions) {
      const item = coords[dimension.id];
      if (item === undefined) throw new Error(`getPosition: no such dimension ${dimension.id}. Coords: ${JSON.stringify(coords)}`);
      const at = dimension.getRootIndexFromRootItem(item);
      if (at === -1) throw new Error(`getPosition: no such item ${item}. Dimension items: ${dimension.getItems()}`);
      position = position * dimension.numItems + at;
    }
    return position;
  }

  _checkCoords(caller, coords) {
    if (this.dimensionIds.some((id) => !coords[id]))
      throw new Error(`${caller}: no value for all dimensions. Dimensions: ${this.dimensionIds}, Coords: ${JSON.stringify(coords)}`);
  }

  setSingleData(measureId, coords, value) {
    this._checkCoords('setSingleData', coords);
    if (this.storedMeasures[measureId] === undefined) throw new Error(`setSingleData: no such stored measure ${measureId}`);
    this.storedMeasures[measureId].setValue(this.getPosition(coords), value);
  }

  getSingleData(measureId, coords) {
    this._checkCoords('getSingleData', coords);
    const position = this.getPosition(coords);
    if (this.storedMeasures[measureId] !== undefined) return this.storedMeasures[measureId].getValue(position);
    if (this.computedMeasures[measureId] === undefined) throw new Error(`getSingleData: no such measure ${measureId}`);
    const expression = this.computedMeasures[measureId];
    const params = {};
    for (const name of expression.variables({ withMembers: true })) params[name] = this.storedMeasures[name].getValue(position);
    return expression.evaluate(params);
  }

  _combinations(dimensionsFilter) {
    const options = {};
    for (const [id, value] of Object.entries(dimensionsFilter)) options[id] = typeof value === 'string' ? [value] : value;
    for (const id of this.dimensionIds) if (dimensionsFilter[id] === undefined) options[id] = this.getDimension(id).getItems();
    return cartesian(options);
  }

  /**
   * src/cube.js:679-707.  A stored measure and a filter whose every combination is valid (./selection.js): one device
   * reduction over the selection, bit for bit the per-cell sum in nesting order.  Anything else takes the per-cell
   * path, for its exact messages.
   */
  getTotalForDimensionItems(measureId, dimensionsFilter = {}) {
    const store = this.storedMeasures[measureId];
    const formula = store === undefined ? this._deviceFormula(measureId) : null;
    if (store !== undefined || formula !== null) {
      const levels = selectionLevels(this.dimensions, dimensionsFilter);
      const lengths = Uint32Array.from(this.dimensions, (d) => d.numItems);
      if (levels.valid && store !== undefined) return store.selectTotal(lengths, levels);
      if (levels.valid) return HipStore.selectTotalFormula(formula.program, formula.stores, lengths, levels);
    }
    return this._getTotalForDimensionItemsPerCell(measureId, dimensionsFilter);
  }

  _getTotalForDimensionItemsPerCell(measureId, dimensionsFilter = {}) {
    return this._combinations(dimensionsFilter).reduce((sum, coords) => sum + this.getSingleData(measureId, coords), 0);
  }

  getDistribution(measureId, dimensionsFilter = {}) {
    const part = this.getTotalForDimensionItems(measureId, dimensionsFilter);
    const whole = this.getTotal(measureId);
    return whole === 0 ? part : part / whole;
  }

  /**
   * src/cube.js:859-888.  Two stored measures and a filter whose every combination is valid: one device scatter, the
   * same cells, values and key order as the per-cell loop.  Anything else takes the per-cell loop (its messages, and
   * the writes it makes before it throws).
   */
  copyMeasureData(sourceMeasureId, targetMeasureId, dimensionsFilter = {}) {
    const source = this.storedMeasures[sourceMeasureId];
    const target = this.storedMeasures[targetMeasureId];
    const formula = source === undefined && target !== undefined ? this._deviceFormula(sourceMeasureId) : null;
    if ((source !== undefined || formula !== null) && target !== undefined) {
      const levels = selectionLevels(this.dimensions, dimensionsFilter);
      if (levels.valid) {
        const copy = copyLevels(levels);
        if (copy.count === 0) return;
        const lengths = Uint32Array.from(this.dimensions, (d) => d.numItems);
        if (source !== undefined) {
          if (target.copySelect(source, lengths, copy)) return;
        } else if (copy.count === levels.count || !formula.stores.includes(target)) {
          // (a selection that revisits cells reads a target input after it was written: cell by cell)
          if (target.copySelectFormula(formula.program, formula.stores, lengths, copy)) return;
        }
      }
    }
    this._copyMeasureDataPerCell(sourceMeasureId, targetMeasureId, dimensionsFilter);
  }

  _copyMeasureDataPerCell(sourceMeasureId, targetMeasureId, dimensionsFilter = {}) {
    for (const coords of this._combinations(dimensionsFilter)) this.setSingleData(targetMeasureId, coords, this.getSingleData(sourceMeasureId, coords));
  }

  /**
   * A computed measure that may run on the device over a selection (DESIGN.md §3 K8): { program, stores } when it is
   * not also stored, reads 1..8 stored measures and nothing else, and compiles to opcodes that give the same bits on
   * the device as getSingleData here (formula.js isDeviceExact).  null: the per-cell path, with its messages.
   */
  _deviceFormula(measureId) {
    const expression = this.computedMeasures[measureId];
    if (expression === undefined || this.storedMeasures[measureId] !== undefined) return null;
    const inputs = {};
    const stores = [];
    for (const name of expression.variables({ withMembers: true })) {
      const store = this.storedMeasures[name];
      if (store === undefined) return null; // `<id>__total` and unknown names: getSingleData throws
      inputs[name] = stores.push(store) - 1;
    }
    if (stores.length === 0 || stores.length > 8) return null;
    const program = expression.compile(inputs);
    if (!isDeviceExact(program) || program.code.length > 96 || program.consts.length > 24 || program.depth > 16) return null;
    return { program, stores };
  }

  // ------------------------------------------------------------------ the derivation helper
  /**
   * Builds the cube that results from replacing the dimension list and running `storeOp` on each
   * stored measure.  `rules`: 'share' (same object, src/cube.js:1011) or a ready-made object.
   */
  _derive(newDimensions, storeOp, rules = 'share', measureFilter = null) {
    const cube = new Cube(newDimensions);
    Object.assign(cube.computedMeasures, this.computedMeasures);
    if (rules === 'share') Object.assign(cube.storedMeasuresRules, this.storedMeasuresRules);
    else cube.storedMeasuresRules = rules;
    for (const id of this.storedMeasureIds) {
      if (measureFilter && !measureFilter(id)) continue;
      cube.storedMeasures[id] = storeOp(this.storedMeasures[id], id);
    }
    return cube;
  }

  /**
   * The reference hands its measures to the store one call at a time (src/cube.js:1012-1020); here two or more stored
   * measures go to their store class TOGETHER where it has the static many-call `name` (HipStore.diceMany, drillUpMany,
   * drillDownMany: one device launch for the measures that can share it).  `call(Store, stores)` returns the new stores
   * in order.  Returns them by measure id — empty for a single measure or a store class without the call: the caller
   * then goes measure by measure.
   */
  _together(ids, name, call) {
    const Store = ids.length >= 2 ? this.storedMeasures[ids[0]].constructor : null;
    const out = {};
    if (!Store || typeof Store[name] !== 'function') return out;
    const results = call(Store, ids.map((id) => this.storedMeasures[id]));
    ids.forEach((id, i) => {
      out[id] = results[i];
    });
    return out;
  }

  /** Pending selections of two or more stored measures are diced together before every measure's cells are needed. */
  _materializeStores() {
    const ids = this.storedMeasureIds;
    const Store = ids.length >= 2 ? this.storedMeasures[ids[0]].constructor : null;
    if (Store && typeof Store.materializeMany === 'function') Store.materializeMany(ids.map((id) => this.storedMeasures[id]));
  }

  _withDimension(index, dimension) {
    const list = this.dimensions.slice();
    list[index] = dimension;
    return list;
  }

  // ------------------------------------------------------------------ drillUp / drillDown
  /** Aggregate one dimension by a parent attribute (minutes by hour, cities by region). */
  drillUp(dimensionId, attribute) {
    const index = this.getDimensionIndex(dimensionId);
    const current = this.dimensions[index];
    if (current.rootAttribute === attribute) return this;
    const rolled = current.drillUp(attribute);
    // eslint-disable-next-line eqeqeq
    if (rolled == current) {
      console.info(`drillUp: no such attribute: ${attribute} in dimension: ${dimensionId} in cube: ${this.dimensionIds.join(', ')}`);
      return this;
    }
    const newDimensions = this._withDimension(index, rolled);
    // the stored measures go to the device together, each with its rule for this dimension (HipStore.drillUpMany)
    const ids = this.storedMeasureIds;
    const rolledUp = this._together(ids, 'drillUpMany', (Store, stores) => Store.drillUpMany(stores, this.dimensions, newDimensions, ids.map((id) => this.storedMeasuresRules[id][dimensionId])));
    return this._derive(newDimensions, (store, id) => rolledUp[id] || store.drillUp(this.dimensions, newDimensions, this.storedMeasuresRules[id][dimensionId]));
  }

  drillDown(dimensionId, attribute) {
    const index = this.getDimensionIndex(dimensionId);
    const current = this.dimensions[index];
    if (current.rootAttribute === attribute) return this;
    const refined = current.drillDown(attribute);
    // eslint-disable-next-line eqeqeq
    if (refined == current) return this;
    const newDimensions = this._withDimension(index, refined);
    const ids = this.storedMeasureIds;
    const refinedStores = this._together(ids, 'drillDownMany', (Store, stores) => Store.drillDownMany(stores, this.dimensions, newDimensions, ids.map((id) => this.storedMeasuresRules[id][dimensionId]), []));
    return this._derive(newDimensions, (store, id) => refinedStores[id] || store.drillDown(this.dimensions, newDimensions, this.storedMeasuresRules[id][dimensionId]));
  }

  // ------------------------------------------------------------------ running aggregates
  /** the checks the calls along a dimension share (`what`: cumulate, rolling); returns the dimension's index */
  _checkAlong(what, dimensionId, attribute) {
    const index = this.getDimensionIndex(dimensionId);
    if (index === -1) throw new Error(`${what}: no such dimension: ${dimensionId}`);
    if (this.dimensions[index].attributes.indexOf(attribute) === -1) throw new Error(`${what}: no such attribute: ${attribute} in dimension: ${dimensionId}`);
    return index;
  }

  _checkCumulate(dimensionId, attribute) {
    return this._checkAlong('cumulate', dimensionId, attribute);
  }

  /**
   * What cumulate and rolling share: the HipStore measures go through many(stores, rules) (null where it does not take
   * one), the rest item by item through perItem(ids); HipStore[pathField] says what ran.
   */
  _alongDimension(dimensionId, pathField, many, perItem) {
    const ids = this.storedMeasureIds;
    const mine = ids.filter((id) => this.storedMeasures[id] instanceof HipStore);
    const made = {};
    HipStore[pathField] = 'per-item';
    if (mine.length > 0) {
      const results = many(mine.map((id) => this.storedMeasures[id]), mine.map((id) => (this.storedMeasuresRules[id] || {})[dimensionId]));
      mine.forEach((id, i) => {
        if (results[i]) made[id] = results[i];
      });
    }
    const rest = ids.filter((id) => !made[id]);
    const launches = HipStore.lastBatchLaunches;
    const chains = rest.length > 0 ? perItem(rest) : null;
    if (HipStore[pathField] === 'device') HipStore.lastBatchLaunches = launches; // (the chains count their own)
    return this._derive(this.dimensions.slice(), (store, id) => made[id] || chains.storedMeasures[id]);
  }

  /**
   * Running aggregates along one dimension (year-to-date, cumulative counts, a running maximum, forward-fill): a new
   * cube with the same dimensions, rules and computed measures in which every stored measure holds, at item i of
   * `dimensionId` (all other coordinates fixed), what
   *   this.dice(dimensionId, root, members).drillUp(dimensionId, attribute)
   * holds in its single item of that dimension, `members` being the items of i's group under `attribute` at positions
   * <= i — by the measure's rule for that dimension.  'all' makes the whole dimension one group; 'year' on a monthly
   * dimension is year-to-date.  An unset cell receives the carried running value; a running value equal to the
   * default is unset and the aggregate restarts.  This cube is untouched.
   * The stored measures go to the device in one call (HipStore.cumulateMany -> olap_store_cumulate_multi, K13); the
   * measures it does not take — order-tracking ones (a `first` / `last` rule), sharded ones, stores of another class —
   * go item by item (_cumulatePerItem, which is also the definition).  HipStore.lastCumulatePath says what ran.
   */
  cumulate(dimensionId, attribute = 'all') {
    const index = this._checkCumulate(dimensionId, attribute);
    if (this.dimensions[index].rootAttribute === attribute) return this.clone(); // every group has one member
    return this._alongDimension(dimensionId, 'lastCumulatePath',
      (stores, rules) => HipStore.cumulateMany(stores, this.dimensions, index, attribute, rules),
      (rest) => this._cumulatePerItem(dimensionId, attribute, rest));
  }

  /**
   * The definition of cumulate, run as written: one dice -> drillUp chain per item of the dimension (2 K launches per
   * measure), each item's rolled-up cells assembled into the result on the host (getData -> setData carries the mask
   * under both defaults).  The path of the measures the device call does not take, and what the tests compare it with.
   */
  _cumulatePerItem(dimensionId, attribute = 'all', measureIds = null) {
    const index = this._checkCumulate(dimensionId, attribute);
    const current = this.dimensions[index];
    const ids = measureIds || this.storedMeasureIds;
    if (current.rootAttribute === attribute) return this.clone(measureIds || []);
    // the chains read only the measures asked for (stores are shared: queries never mutate)
    const source = new Cube(this.dimensions.slice());
    for (const id of ids) {
      source.storedMeasures[id] = this.storedMeasures[id];
      source.storedMeasuresRules[id] = this.storedMeasuresRules[id];
    }
    const items = current.getItems();
    const groups = current.getGroupIndexFromRootIndexMap(attribute);
    const K = items.length;
    const outer = this.dimensions.slice(0, index).reduce((n, d) => n * d.numItems, 1);
    const inner = this.dimensions.slice(index + 1).reduce((n, d) => n * d.numItems, 1);
    const values = {};
    for (const id of ids) values[id] = new Array(outer * K * inner);
    for (let i = 0; i < K; ++i) {
      const members = items.filter((_, j) => j <= i && groups[j] === groups[i]);
      const rolled = source.dice(dimensionId, current.rootAttribute, members).drillUp(dimensionId, attribute);
      for (const id of ids) {
        const cells = rolled.getData(id);
        for (let o = 0; o < outer; ++o) for (let j = 0; j < inner; ++j) values[id][(o * K + i) * inner + j] = cells[o * inner + j];
      }
    }
    return this._derive(this.dimensions.slice(), (store, id) => {
      const rules = this.storedMeasuresRules[id];
      const fresh = store instanceof HipStore ? this._newStore(store._type, store._defaultValue, rules) : new store.constructor(store.size, store._type, store._defaultValue);
      fresh.data = values[id];
      return fresh;
    }, 'share', (id) => ids.includes(id));
  }

  // ------------------------------------------------------------------ rolling windows
  /** the checks rolling and _rollingPerItem share; returns the dimension's index */
  _checkRolling(dimensionId, before, after, attribute) {
    const index = this._checkAlong('rolling', dimensionId, attribute);
    if (!Number.isInteger(before) || !Number.isInteger(after)) throw new Error('rolling: before and after must be integers');
    if (before + after < 0) throw new Error('rolling: empty window');
    return index;
  }

  /**
   * Rolling-window aggregates along one dimension (trailing-12-month totals, a 3-month moving average, a centred
   * maximum): a new cube with the same dimensions, rules and computed measures in which every stored measure holds, at
   * item i of `dimensionId` (all other coordinates fixed), what
   *   this.dice(dimensionId, root, members).drillUp(dimensionId, attribute)
   * holds in its single item of that dimension, `members` being the items j with i - before <= j <= i + after that
   * exist and lie in i's group under `attribute` — by the measure's rule for that dimension.  'all' makes the whole
   * dimension one group.  before and after are integers, either may be negative, before + after >= 0.  A window
   * without members gives an unset cell.  Every window is folded afresh, its set members in ascending order; nothing
   * is subtracted on the way.  This cube is untouched.
   * The stored measures go to the device in one call (HipStore.rollingMany -> olap_store_rolling_multi, K14); the
   * measures it does not take — order-tracking ones (a `first` / `last` rule), sharded ones, stores of another class —
   * go item by item (_rollingPerItem, which is also the definition).  HipStore.lastRollingPath says what ran.
   */
  rolling(dimensionId, before, after = 0, attribute = 'all') {
    const index = this._checkRolling(dimensionId, before, after, attribute);
    return this._alongDimension(dimensionId, 'lastRollingPath',
      (stores, rules) => HipStore.rollingMany(stores, this.dimensions, index, before, after, attribute, rules),
      (rest) => this._rollingPerItem(dimensionId, before, after, attribute, rest));
  }

  /**
   * Item i receives the cell of item i - offset when that item exists and lies in i's group under `attribute`, and is
   * unset otherwise: last month's value beside this month's (offset 1), the same month a year ago (12), a lead
   * (negative).  A window of one item, so the result is the same under every rule.
   */
  shift(dimensionId, offset, attribute = 'all') {
    return this.rolling(dimensionId, offset, 0 - offset, attribute);
  }

  /**
   * The definition of rolling, run as written: one dice -> drillUp chain per item of the dimension whose window has
   * members (2 K launches per measure), assembled on the host as _cumulatePerItem does.  The path of the measures the
   * device call does not take, and what the tests compare it with.
   */
  _rollingPerItem(dimensionId, before, after, attribute = 'all', measureIds = null) {
    const index = this._checkRolling(dimensionId, before, after, attribute);
    const current = this.dimensions[index];
    const ids = measureIds || this.storedMeasureIds;
    const source = new Cube(this.dimensions.slice());
    for (const id of ids) {
      source.storedMeasures[id] = this.storedMeasures[id];
      source.storedMeasuresRules[id] = this.storedMeasuresRules[id];
    }
    const items = current.getItems();
    const groups = current.getGroupIndexFromRootIndexMap(attribute);
    const K = items.length;
    const outer = this.dimensions.slice(0, index).reduce((n, d) => n * d.numItems, 1);
    const inner = this.dimensions.slice(index + 1).reduce((n, d) => n * d.numItems, 1);
    const values = {};
    for (const id of ids) values[id] = new Array(outer * K * inner).fill(this.storedMeasures[id]._defaultValue); // (an empty window: unset)
    for (let i = 0; i < K; ++i) {
      const members = items.filter((_, j) => j >= i - before && j <= i + after && groups[j] === groups[i]);
      if (members.length === 0) continue;
      const rolled = source.dice(dimensionId, current.rootAttribute, members).drillUp(dimensionId, attribute);
      for (const id of ids) {
        const cells = rolled.getData(id);
        for (let o = 0; o < outer; ++o) for (let j = 0; j < inner; ++j) values[id][(o * K + i) * inner + j] = cells[o * inner + j];
      }
    }
    return this._derive(this.dimensions.slice(), (store, id) => {
      const rules = this.storedMeasuresRules[id];
      const fresh = store instanceof HipStore ? this._newStore(store._type, store._defaultValue, rules) : new store.constructor(store.size, store._type, store._defaultValue);
      fresh.data = values[id];
      return fresh;
    }, 'share', (id) => ids.includes(id));
  }

  // ------------------------------------------------------------------ roll-ups of a dimension's groups without a rule
  /**
   * What quantile and _dispersion share.  The stored measures leave in one device call — many(stores): HipStore.quantileMany
   * or varianceMany, null for a measure the call does not take; HipStore[pathField] says what ran — and the rest are
   * computed on the host: host(ids) is the cube of _quantileHost / _varianceHost over those measures.  Returns the new
   * cube over the dimensions of drillUp(dimension `index`, attribute).
   */
  _rollUpAlong(index, attribute, pathField, many, host) {
    const newDimensions = this._withDimension(index, this.dimensions[index].drillUp(attribute));
    const ids = this.storedMeasureIds;
    const made = {};
    HipStore[pathField] = 'host';
    if (ids.length > 0) {
      const results = many(ids.map((id) => this.storedMeasures[id]));
      ids.forEach((id, i) => {
        if (results[i]) made[id] = results[i];
      });
    }
    const rest = ids.filter((id) => !made[id]);
    const onHost = rest.length > 0 ? host(rest) : null;
    return this._derive(newDimensions, (store, id) => {
      if (!made[id]) return onHost.storedMeasures[id];
      // (the device's result is an ordinary store: the order is kept from here on where the rules ask for it, as _newStore does)
      if (Object.values(this.storedMeasuresRules[id] || {}).some((rule) => rule === 'first' || rule === 'last')) made[id].trackOrder();
      return made[id];
    });
  }

  /**
   * What _quantileHost and _varianceHost share: the walk over the output cells of the stored measures `ids`.  For every
   * cell of drillUp(dimension `index`, attribute), cell(v) gets the SET cells of its group's items, in ascending item
   * order, as float64 (v is its own to reorder) and returns the result, or undefined to leave the cell unset.  A result
   * is converted to the store's cell type once (the `data` setter), one equal to the default being unset.  The other
   * measures are shared with this cube.
   */
  _groupCellsHost(index, attribute, ids, cell) {
    const current = this.dimensions[index];
    const rolled = current.drillUp(attribute);
    const newDimensions = this._withDimension(index, rolled);
    const groups = current.getGroupIndexFromRootIndexMap(attribute);
    const K = current.numItems;
    const G = rolled.numItems;
    const outer = this.dimensions.slice(0, index).reduce((n, d) => n * d.numItems, 1);
    const inner = this.dimensions.slice(index + 1).reduce((n, d) => n * d.numItems, 1);
    const members = Array.from({ length: G }, () => []);
    for (let k = 0; k < K; ++k) members[groups[k]].push(k);
    const target = new Cube(newDimensions);
    return this._derive(newDimensions, (store, id) => {
      const cells = store.data;
      const set = new Uint8Array(cells.length); // the status map: the keys of the set cells
      for (const at of store._dataMap.keys()) set[at] = 1;
      const values = new Array(outer * G * inner).fill(store._defaultValue);
      for (let o = 0; o < outer; ++o) {
        for (let g = 0; g < G; ++g) {
          for (let i = 0; i < inner; ++i) {
            const v = [];
            for (const k of members[g]) {
              const at = (o * K + k) * inner + i;
              if (set[at]) v.push(cells[at]);
            }
            const r = cell(v);
            if (r !== undefined) values[(o * G + g) * inner + i] = r;
          }
        }
      }
      const rules = this.storedMeasuresRules[id];
      const fresh = store instanceof HipStore ? target._newStore(store._type, store._defaultValue, rules) : new store.constructor(outer * G * inner, store._type, store._defaultValue);
      fresh.data = values;
      return fresh;
    }, 'share', (id) => ids.includes(id));
  }

  // ------------------------------------------------------------------ order statistics
  /** the checks quantile and _quantileHost share; returns the dimension's index */
  _checkQuantile(dimensionId, attribute, q) {
    const index = this._checkAlong('quantile', dimensionId, attribute);
    if (typeof q !== 'number' || !(q >= 0 && q <= 1)) throw new Error('quantile: q must lie in [0, 1]');
    return index;
  }

  /**
   * Order-statistic roll-up of one dimension (the median day of a month, the p90 of a region): a new cube with the
   * dimensions of drillUp(dimensionId, attribute), the same rules and computed measures, in which every stored
   * measure's cell holds the q-quantile of the SET cells of its group along that dimension, all other coordinates
   * fixed — linear interpolation between the two neighbouring order statistics (_quantileHost is the definition).  The
   * measure's rule for the dimension is not consulted: `median` is not an eighth rule, it is this call.  A group
   * without a set cell gives an unset cell; the root attribute gives a clone (every group has one member).  This cube
   * is untouched.
   * The stored measures go to the device in one call (HipStore.quantileMany -> olap_store_quantile_multi, K15), tracked
   * ones included; sharded measures and stores of another class are selected on the host (_quantileHost).
   * HipStore.lastQuantilePath says what ran.
   */
  quantile(dimensionId, attribute, q) {
    const index = this._checkQuantile(dimensionId, attribute, q);
    if (this.dimensions[index].rootAttribute === attribute) return this.clone();
    return this._rollUpAlong(index, attribute, 'lastQuantilePath',
      (stores) => HipStore.quantileMany(stores, this.dimensions, index, attribute, q),
      (rest) => this._quantileHost(dimensionId, attribute, q, rest));
  }

  /** quantile(dimensionId, attribute, 0.5) */
  median(dimensionId, attribute) {
    return this.quantile(dimensionId, attribute, 0.5);
  }

  /**
   * The definition of quantile, written out; also the path of the measures the device call does not take.  For one
   * output cell: (1) the members are the cells of the group's items that are set, as float64; none: the cell is unset;
   * (2) sorted ascending by the IEEE total order on values (-0 before +0), every NaN last; (3) h = q * (n - 1),
   * lo = floor(h), frac = h - lo; (4) frac > 0: v[lo] + frac * (v[lo + 1] - v[lo]) — one subtraction, one
   * multiplication, one addition — otherwise v[lo]; (5) converted to the store's cell type once (the `data` setter),
   * a result equal to the default being unset.
   */
  _quantileHost(dimensionId, attribute, q, measureIds = null) {
    const index = this._checkQuantile(dimensionId, attribute, q);
    if (this.dimensions[index].rootAttribute === attribute) return this.clone(measureIds || []);
    // NaN last, -0 before +0, the rest by value
    const ascending = (a, b) => {
      if (Number.isNaN(a) || Number.isNaN(b)) return (Number.isNaN(a) ? 1 : 0) - (Number.isNaN(b) ? 1 : 0);
      if (a === b) return (Object.is(a, -0) ? 0 : 1) - (Object.is(b, -0) ? 0 : 1);
      return a < b ? -1 : 1;
    };
    return this._groupCellsHost(index, attribute, measureIds || this.storedMeasureIds, (v) => {
      if (v.length === 0) return undefined;
      v.sort(ascending);
      const h = q * (v.length - 1);
      const lo = Math.floor(h);
      const frac = h - lo;
      let r = v[lo];
      if (frac > 0) {
        const d = v[lo + 1] - r;
        const m = frac * d;
        r += m;
      }
      return r;
    });
  }

  // ------------------------------------------------------------------ dispersion
  /** the checks variance, stddev and _varianceHost share; returns the dimension's index */
  _checkVariance(dimensionId, attribute, ddof) {
    const index = this._checkAlong('variance', dimensionId, attribute);
    if (ddof !== 0 && ddof !== 1) throw new Error('variance: ddof must be 0 or 1');
    return index;
  }

  /**
   * Dispersion roll-up of one dimension (the spread of a day's values within its month, the volatility of a region): a
   * new cube with the dimensions of drillUp(dimensionId, attribute), the same rules and computed measures, in which
   * every stored measure's cell holds the variance of the SET cells of its group along that dimension, all other
   * coordinates fixed — two passes in float64, divided by n - ddof (ddof 0: population, 1: sample); _varianceHost is
   * the definition.  The measure's rule for the dimension is not consulted.  A group with n - ddof <= 0 members gives
   * an unset cell; a variance of 0 is an unset cell under a 0 default and a set 0 under a NaN default; a group that
   * contains ±Infinity or a set NaN gives NaN.  The root attribute is not special: every group has one member.  This
   * cube is untouched.
   * The stored measures go to the device in one call (HipStore.varianceMany -> olap_store_variance_multi, K16), tracked
   * ones included; sharded measures and stores of another class are folded on the host (_varianceHost).
   * HipStore.lastVariancePath says what ran.  On the device, at most 65536 output cells of groups of 1024 members or
   * more are added up by a workgroup each in a fixed tree (the one re-associated form): such a cell may differ from
   * _varianceHost's in the last bits, and is the same on every run.
   */
  variance(dimensionId, attribute, ddof = 0) {
    return this._dispersion(dimensionId, attribute, ddof, 0);
  }

  /** the square root of variance(dimensionId, attribute, ddof), taken in float64 before the one conversion to the cell type */
  stddev(dimensionId, attribute, ddof = 0) {
    return this._dispersion(dimensionId, attribute, ddof, 1);
  }

  /** kind: 0 variance, 1 stddev */
  _dispersion(dimensionId, attribute, ddof, kind) {
    const index = this._checkVariance(dimensionId, attribute, ddof);
    return this._rollUpAlong(index, attribute, 'lastVariancePath',
      (stores) => HipStore.varianceMany(stores, this.dimensions, index, attribute, kind, ddof),
      (rest) => this._varianceHost(dimensionId, attribute, ddof, kind, rest));
  }

  /**
   * The definition of variance (kind 0) and stddev (kind 1), written out; also the path of the measures the device call
   * does not take.  For one output cell: (1) the members are the set cells of the group's items, in ascending item
   * order, as float64 v[0..n); (2) n - ddof <= 0: the cell is unset; (3) s = v[0]; s += v[k]; (4) mean = s / n;
   * (5) m2 = 0; d = v[k] - mean; p = d * d; m2 += p; (6) r = m2 / (n - ddof); (7) stddev: r = Math.sqrt(r) — every
   * operation rounded on its own; a NaN result is the one quiet NaN; (8) converted to the store's cell type once (the
   * `data` setter), a result equal to the default being unset.
   */
  _varianceHost(dimensionId, attribute, ddof, kind, measureIds = null) {
    const index = this._checkVariance(dimensionId, attribute, ddof);
    if (kind !== 0 && kind !== 1) throw new Error('variance: kind must be 0 or 1');
    return this._groupCellsHost(index, attribute, measureIds || this.storedMeasureIds, (v) => {
      const n = v.length;
      if (n - ddof <= 0) return undefined;
      let s = v[0];
      for (let k = 1; k < n; ++k) s += v[k];
      const mean = s / n;
      let m2 = 0;
      for (let k = 0; k < n; ++k) {
        const d = v[k] - mean;
        const p = d * d;
        m2 += p;
      }
      let r = m2 / (n - ddof);
      if (kind === 1) r = Math.sqrt(r);
      return r;
    });
  }

  // ------------------------------------------------------------------ dice / slice
  _diced(index, dimension) {
    // eslint-disable-next-line eqeqeq
    if (dimension == this.dimensions[index]) return this;
    const newDimensions = this._withDimension(index, dimension);
    const diced = this._together(this.storedMeasureIds, 'diceMany', (Store, stores) => Store.diceMany(stores, this.dimensions, newDimensions));
    return this._derive(newDimensions, (store, id) => diced[id] || store.dice(this.dimensions, newDimensions));
  }

  dice(dimensionId, attribute, items, reorder = false) {
    const index = this.getDimensionIndex(dimensionId);
    return this._diced(index, this.dimensions[index].dice(attribute, items, reorder));
  }

  diceRange(dimensionId, attribute, start, end) {
    const index = this.getDimensionIndex(dimensionId);
    return this._diced(index, this.dimensions[index].diceRange(attribute, start, end));
  }

  slice(dimensionId, attribute, value) {
    if (this.getDimensionIndex(dimensionId) === -1) throw new Error(`slice: no such dimension: ${dimensionId}`);
    return this.dice(dimensionId, attribute, [value]).removeDimension(dimensionId);
  }

  collapse() {
    // When every roll-up rule is 'sum', slicing each dimension to 'all' in turn (src/cube.js:320-324)
    // adds up every set cell: that is the store's `total` (in-memory.js:22-28) — one float64
    // reduction per measure instead of one launch per dimension, and without the per-stage rounding
    // to the cell type that a chain of typed stores would add.
    const additive = this.storedMeasureIds.every((id) => this.dimensionIds.every((dimId) => (this.storedMeasuresRules[id][dimId] || 'sum') === 'sum'));
    if (!additive || this.dimensions.length === 0) return this.dimensionIds.reduce((cube, id) => cube.slice(id, 'all', 'all'), this);
    const cube = new Cube([]);
    Object.assign(cube.computedMeasures, this.computedMeasures);
    const rules = deepCopy(this.storedMeasuresRules);
    for (const id of Object.keys(rules)) for (const dimId of this.dimensionIds) delete rules[id][dimId];
    cube.storedMeasuresRules = rules;
    for (const id of this.storedMeasureIds) {
      const source = this.storedMeasures[id];
      const cell = new HipStore(1, source._type, source._defaultValue);
      // under a NaN default an empty measure stays unset; under 0 a zero total unsets itself
      if (!Number.isNaN(source._defaultValue) || source._dataMap.size > 0) cell.setValue(0, source.total);
      cube.storedMeasures[id] = cell;
    }
    return cube;
  }

  aggregateByDimensions(excludeDimensionIds) {
    return this.dimensionIds.filter((id) => !excludeDimensionIds.includes(id)).reduce((cube, id) => cube.slice(id, 'all', 'all'), this);
  }

  getDimensionItemsMap(dimensionIds) {
    const out = {};
    for (const id of this.dimensionIds) if (dimensionIds == null || dimensionIds.includes(id)) out[id] = this.getDimension(id).getItems();
    return out;
  }

  diceByDimensionItems(dimensionItemsMap, measures = [], reorder = false) {
    const newDimensions = this.dimensions.slice();
    for (const [dimensionId, items] of Object.entries(dimensionItemsMap)) {
      const index = this.getDimensionIndex(dimensionId);
      if (index === -1) continue;
      const list = Array.isArray(items) ? items : [items];
      // a dimension literally called 'time' is diced at the periodicity of the given slots (src/cube.js:600-603)
      const attribute = dimensionId === 'time' ? TimeSlot.fromValue(list[0]).periodicity : this.dimensions[index].rootAttribute;
      newDimensions[index] = newDimensions[index].dice(attribute, list, reorder);
    }
    if (newDimensions.every((d, i) => d === this.dimensions[i])) return this;
    const rules = {};
    const wanted = (id) => measures.length === 0 || measures.includes(id);
    for (const id of this.storedMeasureIds.filter(wanted)) rules[id] = deepCopy(this.storedMeasuresRules[id]);
    const diced = this._together(this.storedMeasureIds.filter(wanted), 'diceMany', (Store, stores) => Store.diceMany(stores, this.dimensions, newDimensions));
    return this._derive(newDimensions, (store, id) => diced[id] || store.dice(this.dimensions, newDimensions), rules, wanted);
  }

  /**
   * src/cube.js:811-823.  What every combination receives is a permutation of cells that are already on the device, so
   * the stored measures are regrouped by ONE device call (HipStore.blocksMany, DESIGN.md §3 K11) and every callback gets
   * a cube whose measures are host-resident stores over its block: the same dimension objects, rules and computed
   * measures as diceByDimensionItems(combination) builds.  _scanPerCombination is the reference's loop; it serves a single
   * combination, cubes without stored measures, measures the device call does not take (tracked, sharded, another store
   * class, above its byte cap) and — from the first callback that writes to this cube — the combinations that remain.
   */
  scan(dimensionIds, cb) {
    HipStore.lastBlocksCalls = 0;
    const pass = this._blocksPass(this.getDimensionItemsMap(dimensionIds));
    if (pass === null) {
      this._scanPerCombination(dimensionIds, cb);
      return;
    }
    const diced = this._lazyDice();
    pass.each((combination, blocks) => {
      const newDimensions = this.dimensions.slice();
      for (const [dimensionId, item] of Object.entries(combination)) {
        const index = this.getDimensionIndex(dimensionId);
        newDimensions[index] = diced(index, item);
        // (a dice that does not come down to the one item: the general path decides what the cube looks like)
        if (newDimensions[index].numItems !== 1) return false;
      }
      const cube = new Cube(newDimensions);
      Object.assign(cube.computedMeasures, this.computedMeasures);
      for (const id of pass.ids) {
        cube.storedMeasuresRules[id] = deepCopy(this.storedMeasuresRules[id]);
        cube.storedMeasures[id] = blocks[id];
      }
      cb(cube, combination);
      return true;
    }, (combination) => cb(this.diceByDimensionItems(combination), combination));
  }

  _scanPerCombination(dimensionIds, cb) {
    for (const combination of cartesian(this.getDimensionItemsMap(dimensionIds))) cb(this.diceByDimensionItems(combination), combination);
  }

  /**
   * src/cube.js:815-823.  Every slice(id, 'all', 'all') of aggregateByDimensions rolls up groups of exactly one member,
   * and the seven rules leave a lone value and its set / unset state as they are (in-memory.js:298-331): each callback's
   * cube holds row `c` of the one device pass scan() describes.  Another rule name takes the reference's loop, which
   * throws its message.
   */
  iterateOverDimension(dimension, cb) {
    const others = this.dimensionIds.filter((id) => id !== dimension);
    if (others.length === this.dimensionIds.length) throw new Error(`Cube has no ${dimension} dimension. Dimensions: ${this.dimensionIds}`);
    if (others.length === 0) {
      cb(this, {});
      return;
    }
    HipStore.lastBlocksCalls = 0;
    const known = ['sum', 'average', 'highest', 'lowest', 'first', 'last', 'product'];
    const rulesKnown = this.storedMeasureIds.every((id) => others.every((other) => {
      const rule = (this.storedMeasuresRules[id] || {})[other];
      return rule === undefined || known.includes(rule);
    }));
    const pass = rulesKnown ? this._blocksPass(this.getDimensionItemsMap(others)) : null;
    if (pass === null) {
      this._iterateOverDimensionPerCombination(dimension, cb);
      return;
    }
    const kept = this.getDimension(dimension);
    const diced = this._lazyDice();
    const perCombination = (combination) => cb(this.diceByDimensionItems(combination).aggregateByDimensions([dimension]), combination);
    pass.each((combination, blocks) => {
      // the dimension objects are not handed out, but their dice() may throw: at the same combination as in the loop
      for (const [dimensionId, item] of Object.entries(combination)) if (diced(this.getDimensionIndex(dimensionId), item).numItems !== 1) return false;
      const cube = new Cube([kept]);
      Object.assign(cube.computedMeasures, this.computedMeasures);
      for (const id of pass.ids) {
        const rules = deepCopy(this.storedMeasuresRules[id]);
        if (rules) for (const other of others) delete rules[other];
        cube.storedMeasuresRules[id] = rules;
        cube.storedMeasures[id] = blocks[id];
      }
      cb(cube, combination);
      return true;
    }, perCombination);
  }

  _iterateOverDimensionPerCombination(dimension, cb) {
    const others = this.dimensionIds.filter((id) => id !== dimension);
    if (others.length === this.dimensionIds.length) throw new Error(`Cube has no ${dimension} dimension. Dimensions: ${this.dimensionIds}`);
    if (others.length === 0) {
      cb(this, {});
      return;
    }
    this._scanPerCombination(others, (diced, items) => cb(diced.aggregateByDimensions([dimension]), items));
  }

  /** dimension.dice(attribute, [item]) as diceByDimensionItems calls it for one item, made on first use and kept per (dimension, item). */
  _lazyDice() {
    const made = this.dimensions.map(() => new Map());
    return (index, item) => {
      let dimension = made[index].get(item);
      if (dimension === undefined) {
        // a dimension literally called 'time' is diced at the periodicity of the given slot (src/cube.js:600-603)
        const attribute = this.dimensions[index].id === 'time' ? TimeSlot.fromValue(item).periodicity : this.dimensions[index].rootAttribute;
        dimension = this.dimensions[index].dice(attribute, [item], false);
        made[index].set(item, dimension);
      }
      return dimension;
    };
  }

  /**
   * The one device pass behind scan / iterateOverDimension over the dimensions of `itemsMap` (in cube order, as
   * getDimensionItemsMap lists them), or null where it does not apply: fewer than 2 combinations, no stored measure, more
   * cells per combination than HipStore.blocksMaxBlockCells, a measure that is no HipStore, or HipStore.blocksMany declining.  `each(onBlock, onCombination)` walks the combinations
   * in the order of cartesian(): onBlock(combination, { id: host-resident store over the combination's cells }) while
   * the source cube is as it was when the pass ran (the same store objects, none handed out for writing since; onBlock
   * may return false to decline), onCombination(combination) from then on.
   */
  _blocksPass(itemsMap) {
    const combinations = cartesian(itemsMap);
    const ids = this.storedMeasureIds;
    if (combinations.length < 2 || ids.length === 0) return null;
    // few combinations of very large blocks gain nothing from the one pass (HipStore.blocksMaxBlockCells says on which measurement)
    if (this.storeSize / combinations.length > HipStore.blocksMaxBlockCells) return null;
    const stores = ids.map((id) => this.storedMeasures[id]);
    if (!stores.every((store) => store instanceof HipStore)) return null;
    const flags = this.dimensions.map((d) => itemsMap[d.id] !== undefined);
    const values = HipStore.blocksMany(stores, this.dimensions, flags);
    if (values === null) return null;
    const writes = stores.map((store) => store._writes);
    const rows = this.storeSize / combinations.length;
    const unchanged = () => {
      const now = this.storedMeasureIds;
      return now.length === ids.length && ids.every((id, k) => now[k] === id && this.storedMeasures[id] === stores[k] && stores[k]._writes === writes[k]);
    };
    return {
      ids,
      each: (onBlock, onCombination) => {
        let onePass = true;
        combinations.forEach((combination, c) => {
          onePass = onePass && unchanged();
          if (onePass) {
            const blocks = {};
            ids.forEach((id, k) => {
              const source = stores[k];
              blocks[id] = new HipStore(rows, source._type, source._defaultValue, { host: values[k].subarray(c * rows, (c + 1) * rows), cells: source._cells });
            });
            if (onBlock(combination, blocks) !== false) return;
          }
          onCombination(combination);
        });
      },
    };
  }

  // ------------------------------------------------------------------ dimension list changes
  removeDimension(dimensionId) {
    const rules = deepCopy(this.storedMeasuresRules);
    for (const id of Object.keys(rules)) delete rules[id][dimensionId];
    // the 'all' axis has one item, so dropping it from the list leaves the flat layout unchanged
    const totals = this.drillUp(dimensionId, 'all').storedMeasures;
    const cube = new Cube(this.dimensions.filter((d) => d.id !== dimensionId));
    cube.storedMeasures = totals;
    Object.assign(cube.computedMeasures, this.computedMeasures);
    cube.storedMeasuresRules = rules;
    return cube;
  }

  removeDimensions(dimensionIds) {
    return dimensionIds.reduce((cube, id) => cube.removeDimension(id), this);
  }

  keepDimensions(dimensionIds) {
    return this.dimensionIds.filter((id) => !dimensionIds.includes(id)).reduce((cube, id) => cube.removeDimension(id), this);
  }

  /** Insert a dimension: drillDown from a one-item placeholder to the new items (src/cube.js:910-948). */
  addDimension(newDimension, aggregation = {}, index = null, distributions = {}) {
    const at = index === null ? this.dimensions.length : index;
    const oldDimensions = this.dimensions.slice();
    oldDimensions.splice(at, 0, new CatchAllDimension(newDimension.id, newDimension));
    const newDimensions = oldDimensions.slice();
    newDimensions[at] = newDimension;
    const rules = deepCopy(this.storedMeasuresRules);
    for (const id of Object.keys(rules)) rules[id][newDimension.id] = aggregation[id];
    const ids = this.storedMeasureIds;
    const added = this._together(ids, 'drillDownMany', (Store, stores) => Store.drillDownMany(stores, oldDimensions, newDimensions, ids.map((id) => aggregation[id]), ids.map((id) => distributions[id])));
    return this._derive(newDimensions, (store, id) => added[id] || store.drillDown(oldDimensions, newDimensions, aggregation[id], distributions[id]), rules);
  }

  reorderDimensions(dimensionIds) {
    if (this.dimensions.every((d, i) => dimensionIds[i] === d.id)) return this;
    const newDimensions = dimensionIds.map((id) => this.dimensions.find((d) => d.id === id));
    // (reorderMany dices pending selections together first, as _materializeStores does for the per-measure calls)
    const reordered = this._together(this.storedMeasureIds, 'reorderMany', (Store, stores) => Store.reorderMany(stores, this.dimensions, newDimensions));
    if (Object.keys(reordered).length === 0) this._materializeStores();
    return this._derive(newDimensions, (store, id) => reordered[id] || store.reorder(this.dimensions, newDimensions));
  }

  swapDimensions(dim1, dim2) {
    for (const id of [dim1, dim2]) if (!this.dimensionIds.includes(id)) throw new Error(`swapDimensions: no such dimension ${id}`);
    return this.reorderDimensions(this.dimensionIds.map((id) => (id === dim1 ? dim2 : id === dim2 ? dim1 : id)));
  }

  project(dimensionIds) {
    return this.keepDimensions(dimensionIds).reorderDimensions(dimensionIds);
  }

  // ------------------------------------------------------------------ cube to cube ("next" rows)
  /** Brings this cube onto `targetDims`: project, add missing dims, drill to the target roots, dice. */
  reshape(targetDims) {
    const mine = this.dimensionIds;
    let cube = this.project(targetDims.filter((d) => mine.includes(d.id)).map((d) => d.id));
    targetDims.forEach((target, i) => {
      const actual = cube.dimensions[i];
      if (!actual || actual.id !== target.id) cube = cube.addDimension(target, {}, i);
    });
    targetDims.forEach((target, i) => {
      const actual = cube.dimensions[i];
      if (actual.rootAttribute === target.rootAttribute) return;
      if (actual.attributes.includes(target.rootAttribute)) cube = cube.drillUp(target.id, target.rootAttribute);
      else if (target.attributes.includes(actual.rootAttribute)) cube = cube.drillDown(target.id, target.rootAttribute);
      else throw new Error(`The cube dimensions '${target.id}' are not compatible.`);
      cube = cube.dice(target.id, target.rootAttribute, target.getItems(), true);
    });
    return cube;
  }

  hydrateFromCube(otherCube) {
    let compatible;
    try {
      compatible = otherCube.reshape(this.dimensions);
    } catch (_e) {
      return; // no overlap between the cubes: nothing to load
    }
    // the measures both cubes have go to their store class together where it has loadMany (one device call)
    const ids = this.storedMeasureIds.filter((id) => compatible.storedMeasures[id]);
    const Store = ids.length >= 1 ? this.storedMeasures[ids[0]].constructor : null;
    if (Store && typeof Store.loadMany === 'function') {
      Store.loadMany(ids.map((id) => this.storedMeasures[id]), ids.map((id) => compatible.storedMeasures[id]), this.dimensions, compatible.dimensions);
      return;
    }
    for (const id of ids) this.storedMeasures[id].load(compatible.storedMeasures[id], this.dimensions, compatible.dimensions);
  }

  /** The dimensions both cubes have, each the union or the intersection of the two (src/cube.js:1045-1054). */
  _composedDimensions(otherCube, union) {
    const newDimensions = [];
    for (const dimension of this.dimensions) {
      const other = otherCube.getDimension(dimension.id);
      if (other) newDimensions.push(union ? dimension.union(other) : dimension.intersect(other));
    }
    return newDimensions;
  }

  /**
   * src/cube.js:1040-1080.  The reference creates, fills and hydrates measure by measure (_composePerMeasure); a repeated
   * load changes nothing, and a load into a new (or newly filled) store of the same type and default is a gather, so each
   * source cube is reshaped ONCE and its measures leave in one device call that writes every cell of the new stores once
   * (HipStore.composeMany, DESIGN.md §3 K12).  Tracked (`first` / `last`) and sharded measures, measures of another store
   * class and everything under an addon without the call keep create + fill + load, loaded once per source.
   * HipStore.lastComposeCalls counts the composeMany calls, HipStore.lastBatchLaunches the launches of both kinds.
   */
  compose(otherCube, union = false, fillWith = null) {
    HipStore.lastComposeCalls = 0;
    const cube = new Cube(this._composedDimensions(otherCube, union));
    let launches = 0;
    for (const source of [this, otherCube]) launches += cube._composeFrom(source, fillWith);
    HipStore.lastBatchLaunches = launches;
    Object.assign(cube.computedMeasures, this.computedMeasures, otherCube.computedMeasures);
    return cube;
  }

  /** The stored measures of `source` as measures of this (new) cube; returns the launches the many-calls reported. */
  _composeFrom(source, fillWith) {
    const ids = source.storedMeasureIds;
    const fillOf = (id) => (fillWith && fillWith[id] ? fillWith[id] : undefined);
    const stores = {};
    const create = (id) => {
      const store = source.storedMeasures[id];
      stores[id] = this._newStore(store._type, store._defaultValue, source.storedMeasuresRules[id]);
      if (fillOf(id) !== undefined) stores[id].fill(fillOf(id));
    };
    // the measures that may leave in the one pass are not created here: the pass returns their finished stores
    const ordered = (id) => Object.values(source.storedMeasuresRules[id] || {}).some((rule) => rule === 'first' || rule === 'last');
    const onePass = HipStore.composesMany() && !HipStore.splits(this.dimensions.map((d) => d.numItems));
    const direct = [];
    for (const id of ids) {
      this._checkNewMeasure(id);
      if (onePass && !ordered(id) && source.storedMeasures[id] instanceof HipStore) direct.push(id);
      else create(id);
    }
    let compatible = null;
    try {
      compatible = source.reshape(this.dimensions);
    } catch (_e) {
      // no overlap between the cubes: the measures exist, filled, and nothing is loaded
    }
    let launches = 0;
    const together = compatible ? direct.filter((id) => HipStore.composable(compatible.storedMeasures[id])) : [];
    if (together.length > 0) {
      const made = HipStore.composeMany(together.map((id) => compatible.storedMeasures[id]), this.dimensions, compatible.dimensions, together.map(fillOf));
      together.forEach((id, i) => {
        stores[id] = made[i];
      });
      launches += HipStore.lastBatchLaunches;
    }
    for (const id of direct) if (!stores[id]) create(id);
    const rest = compatible ? ids.filter((id) => !together.includes(id) && compatible.storedMeasures[id]) : [];
    const Store = rest.length >= 1 ? stores[rest[0]].constructor : null;
    if (Store && typeof Store.loadMany === 'function') {
      Store.loadMany(rest.map((id) => stores[id]), rest.map((id) => compatible.storedMeasures[id]), this.dimensions, compatible.dimensions);
      launches += HipStore.lastBatchLaunches;
    } else {
      for (const id of rest) stores[id].load(compatible.storedMeasures[id], this.dimensions, compatible.dimensions);
    }
    for (const id of ids) {
      this.storedMeasures[id] = stores[id];
      this.storedMeasuresRules[id] = source.storedMeasuresRules[id];
    }
    return launches;
  }

  /** compose as the reference orders its calls: one hydrateFromCube per measure (the comparison path of compose). */
  _composePerMeasure(otherCube, union = false, fillWith = null) {
    const cube = new Cube(this._composedDimensions(otherCube, union));
    for (const source of [this, otherCube]) {
      for (const id of source.storedMeasureIds) {
        const store = source.storedMeasures[id];
        cube.createStoredMeasure(id, source.storedMeasuresRules[id], store._type, store._defaultValue);
        if (fillWith && fillWith[id]) cube.fillData(id, fillWith[id]);
        cube.hydrateFromCube(source);
      }
    }
    Object.assign(cube.computedMeasures, this.computedMeasures, otherCube.computedMeasures);
    return cube;
  }

  // ------------------------------------------------------------------ wire format ("next" row f3)
  /** Same container as the reference (src/cube.js:1135-1151); computed measures are not carried. */
  serialize() {
    this._materializeStores();
    return toBuffer({
      dimensions: this.dimensions.map((d) => d.serialize()),
      storedMeasuresKeys: this.storedMeasureIds,
      storedMeasures: Object.values(this.storedMeasures).map((store) => store.serialize()),
      storedMeasuresRules: this.storedMeasuresRules,
      computedMeasures: this.computedMeasureIds.reduce((out, id) => {
        out[id] = this.computedMeasures[id].toString();
        return out;
      }, {}),
    });
  }

  serializeToBase64String() {
    return Buffer.from(this.serialize()).toString('base64');
  }

  static deserialize(buffer) {
    const GenericDimension = require('./dimension/generic');
    const TimeDimension = require('./dimension/time');
    const data = fromBuffer(buffer);
    // a time dimension's record carries `start` (src/dimension/factory.js:6-12)
    const cube = new Cube(data.dimensions.map((blob) => (fromBuffer(blob).start ? TimeDimension.deserialize(blob) : GenericDimension.deserialize(blob))));
    cube.storedMeasuresRules = data.storedMeasuresRules || {};
    data.storedMeasuresKeys.forEach((id, i) => {
      cube.storedMeasures[id] = HipStore.deserialize(data.storedMeasures[i]);
      // (a blob whose cells are not listed in ascending order keeps that order by itself, olap_store_from_sparse)
      if (Object.values(cube.storedMeasuresRules[id] || {}).some((rule) => rule === 'first' || rule === 'last')) cube.storedMeasures[id].trackOrder();
    });
    for (const id of Object.keys(data.computedMeasures || {})) cube.computedMeasures[id] = getParser().parse(data.computedMeasures[id]);
    return cube;
  }

  static deserializeFromBase64String(text) {
    return Cube.deserialize(toArrayBuffer(Buffer.from(text, 'base64')));
  }
}

module.exports = Cube;
