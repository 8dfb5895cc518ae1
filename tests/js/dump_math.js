'use strict';
// Reads one JSON document from stdin: a list of jobs { fn, args }, where `args` holds one list of hex-encoded doubles (16
// digits, big-endian bits) per argument and `fn` is either the name of a Math function or 'f:' followed by a formula over
// a, b, c for js/formula.js's evaluate().  Prints, per job, the results cell by cell as hex-encoded doubles (one JSON
// document), for tests/test_formula_reference.py to compare with tests/formula_reference.py.
const { getParser } = require('../../olap-in-memory_amd/js/formula');

const view = new DataView(new ArrayBuffer(8));
const decode = (hex) => {
  view.setUint32(0, parseInt(hex.slice(0, 8), 16));
  view.setUint32(4, parseInt(hex.slice(8), 16));
  return view.getFloat64(0);
};
const encode = (x) => {
  view.setFloat64(0, x);
  return view.getUint32(0).toString(16).padStart(8, '0') + view.getUint32(4).toString(16).padStart(8, '0');
};

const jobs = JSON.parse(require('fs').readFileSync(0, 'utf8'));
const out = jobs.map(({ fn, args }) => {
  const columns = args.map((column) => column.map(decode));
  let apply;
  if (fn.startsWith('f:')) {
    const expression = getParser().parse(fn.slice(2));
    apply = (a, b, c) => expression.evaluate({ a, b, c });
  } else {
    apply = (...xs) => Math[fn](...xs);
  }
  return columns[0].map((_x, i) => encode(apply(...columns.map((column) => column[i]))));
});
console.log(JSON.stringify(out));
