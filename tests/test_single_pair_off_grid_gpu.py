"""olap_plan_run on ONE buffer pair whose pointers are one cell off the 16-byte grid, one case per form of the gather
family (dice, the fused dice -> drillUp, reorder, load, the row forms of drillDown).  A single pair goes through the
family's launchers as a batch of one; off the grid the plan's 16-byte lanes are not available, and what a form does then differs:

  gather, gather_reduce, load_scatter (lanes)   one cell per lane
  dice_direct                                   needs only the OUTPUT on the grid; off it the plan falls to gather
  reorder_brick4 (4-byte cells)                 the scalar brick kernel over the same bricks
  load_scatter_run                              needs only HIS side on the grid; off it the per-cell scatter
  load_permute_rows                             the same kernel: its 16-byte accesses ask for the cell's own alignment only
  drilldown_rows_lines                          needs every buffer on the grid; off it drilldown_rows, one cell per lane

Which kernel ran cannot be seen from here; what is pinned is what it leaves: the cells the CPU oracle computes, bit for
bit the cells the same plan leaves in aligned buffers, and nothing written before or after the pair's range.  One cell
off is 4 bytes for float32 cells and every mask, 8 bytes for float64 cells."""
import numpy as np
import pytest

from conftest import load_package
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
Plan = pkg.hipstore.Plan

GUARD = 8  # sentinel cells before and after a pair's range (a whole number of 16-byte groups in every cell type)
SENTINEL = {"float32": -777.0, "float64": -777.0, "int32": 0x55555555}
ROWS, LINES = "drilldown_rows_kernel", "drilldown_rows_lines_kernel"


def ident(n):
    return list(range(n))


def dice_case(old, new, sel, kernel, offsets=((1, 1),)):
    return dict(n_in=int(np.prod(old)), n_out=int(np.prod(new)), kernel=kernel, offsets=offsets,
                plan=lambda dtype: Plan.dice(dtype, 0.0, old, new, sel),
                oracle=lambda src, dst: src.dice(old, new, sel))


def fused_case(rule):
    old, mid, new = [6, 10, 8], [1, 10, 8], [1, 3, 8]  # slice dimension 0 to one item, roll dimension 1 up into 4 + 3 + 3
    sel, maps = [[4], ident(10), ident(8)], [[0], [0, 0, 0, 0, 1, 1, 1, 2, 2, 2], ident(8)]
    return dict(n_in=int(np.prod(old)), n_out=int(np.prod(new)), kernel="gather_reduce_kernel", offsets=((1, 1),),
                plan=lambda dtype: Plan.dice_drillup(dtype, 0.0, rule, old, mid, new, sel, maps),
                oracle=lambda src, dst: src.dice(old, mid, sel).drill_up(mid, new, maps, rule))


def reorder_case(lens, perm):
    n = int(np.prod(lens))  # (the kernel depends on the cell size and on the masks: without masks the two-axis transpose runs)
    return dict(n_in=n, n_out=n, kernel=None, offsets=((1, 1),),
                plan=lambda dtype: Plan.reorder(dtype, 0.0, lens, perm),
                oracle=lambda src, dst: src.reorder(lens, perm))


def load_case(my_len, his_len, maps, kernel, offsets=((1, 1),)):
    def loaded(src, dst):
        dst.load(src, my_len, his_len, maps)
        return dst

    # `in` is the other store, `out` this one: (0, 1) is off the grid on my side only
    return dict(n_in=int(np.prod(his_len)), n_out=int(np.prod(my_len)), kernel=kernel, offsets=offsets,
                plan=lambda dtype: Plan.load(dtype, 0.0, 0.0, my_len, his_len, maps), oracle=loaded)


def drilldown_case(width, kernel):
    old, new = [2, 3, width], [2, 7, width]  # dimension 1 from 3 parents to 3 + 2 + 2 children
    maps = [ident(2), [0, 0, 0, 1, 1, 2, 2], ident(width)]
    return dict(n_in=int(np.prod(old)), n_out=int(np.prod(new)), kernel=kernel, offsets=((1, 1),),
                plan=lambda dtype: Plan.drilldown(dtype, 0.0, "sum", old, new, maps),
                oracle=lambda src, dst: src.drill_down(old, new, maps, "sum"))


CASES = {
    "gather-middle": dice_case([6, 5, 8], [6, 4, 8], [ident(6), [4, 2, -1, 0], ident(8)], "gather"),
    "gather-two-dimensions": dice_case([5, 3, 7], [3, 3, 4], [[4, 0, 2], ident(3), [6, 1, 0, 3]], "gather"),
    # only the input off the grid, then the output too (which must fall to gather)
    "dice-direct": dice_case([30, 5, 7], [30, 4, 7], [ident(30), [4, 2, -1, 0], ident(7)], "dice_direct_kernel", offsets=((1, 0), (1, 1))),
    "fused-sum": fused_case("sum"),
    "fused-highest": fused_case("highest"),
    "reorder-reversed": reorder_case([12, 7, 20], [2, 1, 0]),
    "reorder-transposed": reorder_case([37, 53], [1, 0]),
    # trailing dimensions kept: 16-byte lanes
    "load-lanes": load_case([6, 8, 12], [4, 8, 12], [[4, -1, 0, 2], ident(8), ident(12)], "load_scatter (16-byte lanes)"),
    # the innermost dimension remapped: off the grid on my side only, then on his side too (the per-cell form)
    "load-runs": load_case([4, 10], [6, 10], [[3, -1, 0, 2, -1, 1], [9, 3, 0, 7, 1, 8, 2, 6, 4, 5]], "load_scatter (16-byte runs of the other store)",
                           offsets=((0, 1), (1, 1))),
    "load-permuted-rows": load_case([5, 7], [5, 7], [ident(5), [3, 0, 6, 1, 5, 2, 4]], "load_permute_rows_kernel"),
    "drilldown-rows": drilldown_case(1056, ROWS),
    "drilldown-lines": drilldown_case(516, LINES),
    "drilldown-lines-odd-rows": drilldown_case(515, LINES),
}


def cells(rng, n, dtype):
    """small integers (every result is exact), a third of the cells unset: 0 under the 0 default, mask word 0"""
    vals = rng.integers(1, 7, size=n).astype(dtype)
    unset = rng.random(n) < 0.33
    vals[unset] = 0
    return vals, np.where(unset, 0, 2).astype(np.int32)


def oracle_of(vals, dtype):
    o = OracleStore(vals.size, dtype, 0.0)
    o.set_data(vals.astype(np.float64))
    return o


def place(torch, arr, off):
    """`arr` in device memory, its first cell `off` cells past a 16-byte boundary, sentinel cells all around it
    -> (the buffer, the index of the first cell, its address)"""
    first = GUARD + off
    host = np.full(first + arr.size + 2 * GUARD - off, SENTINEL[arr.dtype.name], arr.dtype)
    host[first:first + arr.size] = arr
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, first, t.data_ptr() + first * arr.itemsize


def lift(t, first, n):
    """the pair's n cells, after checking that the sentinels around them are untouched"""
    host = t.cpu().numpy()
    sentinel = np.asarray(SENTINEL[host.dtype.name], host.dtype)
    assert (host[:first] == sentinel).all(), "cells before the pair's range were written"
    assert (host[first + n:] == sentinel).all(), "cells after the pair's range were written"
    return host[first:first + n].copy()


def run_pair(torch, plan, src, dst, in_off, out_off, masks):
    """plan.run over (src -> dst), each a (values, mask) of host arrays -> what the output range holds afterwards"""
    t_in, _, p_in = place(torch, src[0], in_off)
    t_out, first, p_out = place(torch, dst[0], out_off)
    p_sin = p_sout = None
    if masks:
        t_sin, _, p_sin = place(torch, src[1], in_off)
        t_sout, s_first, p_sout = place(torch, dst[1], out_off)
    torch.cuda.synchronize()
    plan.run(p_in, p_sin, p_out, p_sout)
    pkg.capi.check(pkg.lib().olap_device_synchronize())
    torch.cuda.synchronize()
    n = dst[0].size
    assert lift(t_in, GUARD + in_off, src[0].size).tobytes() == src[0].tobytes()  # the input is only read
    return lift(t_out, first, n), (lift(t_sout, s_first, n) if masks else None)


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "no-masks"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", list(CASES))
def test_a_single_pair_off_the_16_byte_grid(case, dtype, masks):
    import torch

    c = CASES[case]
    plan = c["plan"](dtype)
    if c["kernel"]:
        assert c["kernel"] in plan.kernel_name, plan.kernel_name
    rng = np.random.default_rng(40)
    src, dst = cells(rng, c["n_in"], dtype), cells(rng, c["n_out"], dtype)  # (what dst holds matters to load alone)
    want_v, want_s = c["oracle"](oracle_of(src[0], dtype), oracle_of(dst[0], dtype)).typed()
    base_v, base_s = run_pair(torch, plan, src, dst, 0, 0, masks)
    print(case, dtype, masks, "aligned: cells that differ from the oracle:", int((base_v != want_v).sum()))
    assert base_v.tobytes() == want_v.tobytes()
    assert not masks or np.array_equal(base_s, want_s)
    for in_off, out_off in c["offsets"]:
        got_v, got_s = run_pair(torch, plan, src, dst, in_off, out_off, masks)
        print(case, dtype, masks, (in_off, out_off), "cells that differ from the oracle:", int((got_v != want_v).sum()),
              "from the aligned run:", int((got_v != base_v).sum()))
        assert got_v.tobytes() == want_v.tobytes(), (in_off, out_off)
        assert got_v.tobytes() == base_v.tobytes(), (in_off, out_off)
        if masks:
            assert np.array_equal(got_s, want_s), (in_off, out_off)
            assert np.array_equal(got_s, base_s), (in_off, out_off)
