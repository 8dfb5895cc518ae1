'use strict';
/*
 * The cartesian selection of a dimensions filter as LEVELS (include/olap_hip.h, olap_store_select_total), with no
 * device work: what Cube.getTotalForDimensionItems / copyMeasureData (the reference's src/cube.js:679-707, :859-888)
 * enumerate through getCombinations (:19-32), combination by combination.
 *
 *   - a string filter value is a one-item list;
 *   - the filter's keys come first, in their own (Object.keys) order, then the cube's unfiltered dimensions in cube
 *     order with all their items; the first key is the outermost;
 *   - repeats are visited twice; a key that is not a dimension of the cube multiplies the combinations (axis -1);
 *     an empty list gives no combination.
 *
 * `valid` is false when the per-cell path would throw for some combination (a dimension without a value, an unknown
 * item, a value that is neither a string nor an array): the caller then runs that path, for its exact message and
 * the writes it makes before the throw.
 */

// all items of an unfiltered dimension, resolved as getPosition resolves them (a repeated item keeps its last index)
const resolvedItems = new WeakMap();
function allItems(dimension) {
  const items = dimension.getItems();
  const hit = resolvedItems.get(dimension);
  if (hit && hit.items === items && hit.list.length === items.length) return hit;
  const list = new Int32Array(items.length);
  let valid = true;
  for (let j = 0; j < items.length; ++j) {
    const at = items[j] ? dimension.getRootIndexFromRootItem(items[j]) : -1;
    if (at === -1) valid = false;
    list[j] = at;
  }
  const entry = { items, list, valid };
  resolvedItems.set(dimension, entry);
  return entry;
}

/**
 * selectionLevels(dimensions, filter) -> { axis: Int32Array, lists: Int32Array[], valid, count }
 * axis[l]: index of the level's dimension in `dimensions`, or -1 for a key that is not one (its list holds zeros:
 * only its length matters); count: the number of combinations.
 */
function selectionLevels(dimensions, filter = {}) {
  const ids = dimensions.map((d) => d.id);
  const options = {};
  for (const [id, value] of Object.entries(filter)) options[id] = typeof value === 'string' ? [value] : value;
  for (const id of ids) if (filter[id] === undefined) options[id] = null; // (all items, at the key's own position)
  const keys = Object.keys(options);
  const axis = new Int32Array(keys.length);
  const lists = new Array(keys.length);
  let valid = true;
  let count = 1;
  keys.forEach((key, l) => {
    const d = ids.indexOf(key);
    const value = options[key];
    axis[l] = d;
    if (d >= 0 && filter[key] === undefined) {
      const all = allItems(dimensions[d]);
      if (!all.valid) valid = false;
      lists[l] = all.list;
    } else if (!Array.isArray(value)) {
      valid = false;
      lists[l] = new Int32Array(0);
    } else if (d < 0) {
      lists[l] = new Int32Array(value.length);
    } else {
      const list = new Int32Array(value.length);
      for (let j = 0; j < value.length; ++j) {
        const item = value[j];
        const at = item ? dimensions[d].getRootIndexFromRootItem(item) : -1;
        if (at === -1) valid = false;
        list[j] = at;
      }
      lists[l] = list;
    }
    count *= lists[l].length;
  });
  return { axis, lists, valid, count };
}

/**
 * The levels of a copy: repeats removed (first occurrence kept: setValue of the same cell twice changes nothing) and
 * keys that are not dimensions dropped, so that every combination is one distinct cell, in nesting order.
 */
function copyLevels(levels) {
  const axis = [];
  const lists = [];
  levels.axis.forEach((d, l) => {
    if (d < 0) return;
    const seen = new Set();
    const out = [];
    for (const at of levels.lists[l]) {
      if (seen.has(at)) continue;
      seen.add(at);
      out.push(at);
    }
    axis.push(d);
    lists.push(Int32Array.from(out));
  });
  const empty = levels.lists.some((list) => list.length === 0);
  return { axis: Int32Array.from(axis), lists, valid: levels.valid, count: empty ? 0 : lists.reduce((n, list) => n * list.length, 1) };
}

module.exports = { selectionLevels, copyLevels };
