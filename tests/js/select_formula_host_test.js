'use strict';
/*
 * ../../olap-in-memory_amd/js/formula.js isDeviceExact without a GPU: the formulas whose every opcode gives the same
 * bits on the device as evaluate() here take the device route of getTotalForDimensionItems / copyMeasureData; the
 * rest (round, ^, roundTo, transcendental ops, hypot, atan2, cbrt, `<id>__total`) keep the per-cell path.
 */
const { describe, it, assert, run } = require('./harness');
const { getParser, isDeviceExact, DEVICE_EXACT_OPS, OP } = require('../../olap-in-memory_amd/js/formula');

const compile = (text) => {
  const expression = getParser().parse(text);
  const inputs = {};
  const scalars = {};
  for (const name of expression.variables()) {
    if (name.includes('__total')) scalars[name] = Object.keys(scalars).length;
    else inputs[name] = Object.keys(inputs).length;
  }
  return expression.compile(inputs, scalars);
};

describe('isDeviceExact', () => {
  it('the exact set', () => {
    const names = ['CONST', 'INPUT', 'ADD', 'SUB', 'MUL', 'DIV', 'MOD', 'NEG', 'NANADD', 'SELECT', 'MIN', 'MAX', 'ISNAN', 'ABS', 'CEIL', 'FLOOR',
      'TRUNC', 'SQRT', 'SIGN', 'NOT'];
    assert.deepEqual(Array.from(DEVICE_EXACT_OPS).sort((x, y) => x - y), names.map((n) => OP[n]).sort((x, y) => x - y));
  });

  it('formulas inside the set', () => {
    for (const text of ['routers / antennas', 'a + b', 'a - b * c % 3', '-a || b', 'a ? b : 2', 'min(a, b, 4)', 'max(a, -b)', 'isNaN(a)',
      'abs a + ceil(b) - floor(c)', 'trunc(a / 3)', 'sqrt(a)', 'sign(a - b)', 'not a', 'if(a, b, c)', 'hypot(a)', 'PI * a', 'true + a'])
      assert.ok(isDeviceExact(compile(text)), text);
  });

  it('formulas outside the set', () => {
    for (const text of ['round(a)', 'a ^ 2', 'pow(a, b)', 'roundTo(a, 2)', 'sin(a)', 'cos a', 'tan(a)', 'asin(a)', 'acos(a)', 'atan(a)',
      'atan2(a, b)', 'hypot(a, b)', 'cbrt(a)', 'exp(a)', 'ln(a)', 'log(a)', 'log10(a)', 'log2(a)', 'a / a__total', 'a + round(b)'])
      assert.ok(!isDeviceExact(compile(text)), text);
  });

  it('operand words are not read as opcodes', () => {
    // INPUT 23 (ROUND's code) and CONST 32 (SIN's code) are operands, not operations
    assert.ok(isDeviceExact({ code: Int32Array.of(OP.INPUT, OP.ROUND, OP.CONST, OP.SIN, OP.ADD) }));
    assert.ok(!isDeviceExact({ code: Int32Array.of(OP.INPUT, 0, OP.ROUND) }));
  });
});

run();
