// Developer tool: the host side of olap_store_blocks_report (csrc/olap_blocks.hip) under AddressSanitizer + UBSan, as a
// stand-alone program — no device, nothing loaded into another process:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tools/blocks_plan_check.hip -o /tmp/blocks_plan_check && /tmp/blocks_plan_check
//
// It includes the translation unit itself, with stand-ins for what the library's other units provide, and checks
//   * the argument refusals, in their order, over store handles without buffers;
//   * plan_blocks for many shapes and flag sets: the index arithmetic of the two kernels, restated on the host over the
//     plan's tables (every workgroup, every lane), writes every cell of the result exactly once, inside it, and puts
//     the cell numpy's reshape(lens).transpose(scanned + kept) puts there.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../olap-in-memory_amd/csrc/olap_blocks.hip"

static char g_error[512];
int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t, const char *what) { return fail(OLAP_ERR_HIP, "%s", what); }
hipError_t dev_alloc(void **, size_t) { return hipErrorOutOfMemory; }
void dev_free(void *) {}
int require_device() { return fail(OLAP_ERR_NO_DEVICE, "no device"); }
bool mask_is_primary(const olap_store *s) { return s->default_kind == OLAP_DEFAULT_NAN && (s->dtype == OLAP_INT32 || s->dtype == OLAP_UINT32); }

static int failures = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      ++failures;                  \
      printf("FAIL %s: ", #cond);  \
      printf(__VA_ARGS__);         \
      printf("\n");                \
    }                              \
  } while (0)

// the kernels' index arithmetic over the plan, on the host: out[where a cell goes] = the cell's flat index in the store
static void run_plan(const BlocksPlan &p, uint64_t size, int vec, std::vector<int64_t> &out, std::vector<int> &writes) {
  if (!p.transpose) {
    const BlockDims &m = p.dims;
    const int V = p.row % vec == 0 ? vec : 1;
    for (uint64_t t = 0; t < size / V; ++t) {
      uint32_t c = (uint32_t)t * V;
      uint64_t other = 0;
      for (int d = m.nd - 1; d >= 0; --d) {
        const uint32_t q = c / m.len[d];
        other += (uint64_t)(c - q * m.len[d]) * (m.by_result ? m.src_stride[d] : m.dst_stride[d]);
        c = q;
      }
      const uint64_t src = m.by_result ? other : t * V, dst = m.by_result ? t * V : other;
      for (int e = 0; e < V; ++e) {
        EXPECT(src + e < size, "a read at %llu of %llu cells", (unsigned long long)(src + e), (unsigned long long)size);
        out.at(dst + e) = (int64_t)(src + e), ++writes.at(dst + e);
      }
    }
    return;
  }
  const BlockDims &m = p.dims;
  const BlockTiles &t = p.tiles;
  uint64_t groups = (uint64_t)t.tiles_x * t.tiles_y;
  for (int d = 0; d < m.nd; ++d) groups *= m.len[d];
  std::vector<int64_t> tile((size_t)kBlockTile * (kBlockTile + 1));
  for (uint64_t g = 0; g < groups; ++g) {
    uint32_t w = (uint32_t)g;
    const uint32_t bx = w % t.tiles_x;
    w /= t.tiles_x;
    const uint32_t by = w % t.tiles_y;
    w /= t.tiles_y;
    uint64_t src = 0, dst = 0;
    for (int d = m.nd - 1; d >= 0; --d) {
      const uint32_t q = w / m.len[d], digit = w - q * m.len[d];
      src += (uint64_t)digit * m.src_stride[d];
      dst += (uint64_t)digit * m.dst_stride[d];
      w = q;
    }
    const uint32_t x0 = bx * t.tx, y0 = by * t.ty, pitch = t.tx + 1;
    std::fill(tile.begin(), tile.end(), -1);
    for (uint32_t lane = 0; lane < (uint32_t)kBlock; ++lane) {
      const uint32_t x = lane % t.tx;
      for (uint32_t y = lane / t.tx; y < t.ty; y += kBlock / t.tx)
        if (x0 + x < t.lx && y0 + y < t.ly) {
          const uint64_t at = src + (uint64_t)(y0 + y) * t.src_y + (x0 + x);
          EXPECT(at < size, "a read at %llu of %llu cells", (unsigned long long)at, (unsigned long long)size);
          tile.at(y * pitch + x) = (int64_t)at;
        }
    }
    for (uint32_t lane = 0; lane < (uint32_t)kBlock; ++lane) {
      const uint32_t y = lane % t.ty;
      for (uint32_t x = lane / t.ty; x < t.tx; x += kBlock / t.ty)
        if (x0 + x < t.lx && y0 + y < t.ly) {
          const uint64_t at = dst + (uint64_t)(x0 + x) * t.dst_x + (y0 + y);
          out.at(at) = tile.at(y * pitch + x), ++writes.at(at);
        }
    }
  }
}

static void check_shape(const std::vector<uint32_t> &lens, const std::vector<uint8_t> &flags) {
  const int nd = (int)lens.size();
  uint64_t size = 1, kept = 1;
  for (int d = 0; d < nd; ++d) size *= lens[d], kept *= flags[d] ? 1 : lens[d];
  const BlocksPlan p = plan_blocks(nd, lens.data(), flags.data(), kept);  // (main runs every shape with and without OLAP_BLOCKS_BY_STORE)
  // the transposition, dimension by dimension: [scanned..., kept...] row-major
  std::vector<int> order;
  for (int d = 0; d < nd; ++d) if (flags[d]) order.push_back(d);
  for (int d = 0; d < nd; ++d) if (!flags[d]) order.push_back(d);
  std::vector<uint64_t> stride(nd);
  uint64_t s = 1;
  for (int d = nd - 1; d >= 0; --d) stride[d] = s, s *= lens[d];
  for (int vec : {4, 2}) {
    std::vector<int64_t> out(size, -1);
    std::vector<int> writes(size, 0);
    run_plan(p, size, vec, out, writes);
    for (uint64_t i = 0; i < size; ++i) {
      uint64_t rest = i, at = 0;
      for (int k = nd - 1; k >= 0; --k) at += (rest % lens[order[k]]) * stride[order[k]], rest /= lens[order[k]];
      if (writes[i] != 1 || out[i] != (int64_t)at) {
        EXPECT(false, "shape of %d dimensions, result cell %llu: written %d times, holds %lld, wants %llu", nd, (unsigned long long)i, writes[i],
               (long long)out[i], (unsigned long long)at);
        return;
      }
    }
  }
}

static olap_store fake(uint64_t size, int device = 0, bool tracked = false) {
  olap_store s{};
  s.size = size, s.dtype = OLAP_FLOAT32, s.default_kind = OLAP_DEFAULT_ZERO, s.device = device, s.track_order = tracked;
  return s;
}

int main() {
  // refusals, in order (the messages: tests/test_scan_blocks_host.py)
  olap_store a = fake(6), b = fake(6), eight = fake(8), far = fake(6, 1), tracked = fake(6, 0, true);
  const uint32_t lens[2] = {2, 3};
  const uint8_t first[2] = {1, 0}, none[2] = {0, 0};
  double result[16];
  int launches = -1;
  const olap_store *ok[2] = {&a, &b}, *null_entry[2] = {&a, nullptr}, *wrong_size[2] = {&a, &eight}, *two_devices[2] = {&a, &far}, *ordered[2] = {&a, &tracked};
  EXPECT(olap_store_blocks_report(2, nullptr, 2, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT, "%s", g_error);
  EXPECT(olap_store_blocks_report(-1, ok, 2, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT, "%s", g_error);
  EXPECT(olap_store_blocks_report(2, null_entry, 2, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT && strstr(g_error, "store 1"), "%s", g_error);
  EXPECT(olap_store_blocks_report(2, ok, 33, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT && strstr(g_error, "ndim 33"), "%s", g_error);
  EXPECT(olap_store_blocks_report(2, ok, 2, nullptr, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT, "%s", g_error);
  EXPECT(olap_store_blocks_report(2, ok, 2, lens, nullptr, result, &launches) == OLAP_ERR_INVALID_ARGUMENT, "%s", g_error);
  EXPECT(olap_store_blocks_report(2, wrong_size, 2, lens, none, result, &launches) == OLAP_ERR_INVALID_ARGUMENT && strstr(g_error, "no dimension"), "%s", g_error);
  EXPECT(olap_store_blocks_report(2, wrong_size, 2, lens, first, result, &launches) == OLAP_ERR_LENGTH_MISMATCH, "%s", g_error);
  EXPECT(olap_store_blocks_report(2, two_devices, 2, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT && strstr(g_error, "devices"), "%s", g_error);
  EXPECT(olap_store_blocks_report(2, ordered, 2, lens, first, result, &launches) == OLAP_ERR_INVALID_ARGUMENT && strstr(g_error, "ordered:") == g_error, "%s", g_error);
  EXPECT(olap_store_blocks_report(2, ok, 2, lens, first, result, &launches) == OLAP_ERR_NO_DEVICE && launches == 0, "%s", g_error);
  EXPECT(olap_store_blocks_report(0, nullptr, 2, lens, first, nullptr, &launches) == OLAP_OK, "%s", g_error);
  // 32 dimensions of 2^32 - 1 items: the products saturate instead of wrapping
  uint32_t huge[OLAP_MAX_DIMS];
  uint8_t every[OLAP_MAX_DIMS];
  for (int d = 0; d < OLAP_MAX_DIMS; ++d) huge[d] = 0xFFFFFFFFu, every[d] = (uint8_t)(d & 1);
  EXPECT(olap_store_blocks_report(2, ok, OLAP_MAX_DIMS, huge, every, result, &launches) == OLAP_ERR_LENGTH_MISMATCH, "%s", g_error);

  // plans: every flag set of these shapes (a flag set without a scanned dimension is refused before a plan is made)
  const std::vector<std::vector<uint32_t>> shapes = {{3, 5, 7},   {65, 3, 67}, {2, 3, 2, 3, 2, 3}, {1, 5, 1, 4}, {7}, {1, 1},      {129, 66}, {66, 129},
                                                     {4, 8, 12},  {12, 100, 5}, {5, 100, 12},      {2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2}, {64, 64},  {63, 1, 65}};
  int plans = 0;
  for (int by_store = 0; by_store < 2; ++by_store) {
    if (by_store) setenv("OLAP_BLOCKS_BY_STORE", "1", 1);
    for (const auto &shape : shapes) {
      const int nd = (int)shape.size();
      for (uint32_t bits = 1; bits < (1u << nd); ++bits) {
        std::vector<uint8_t> flags(nd);
        for (int d = 0; d < nd; ++d) flags[d] = (bits >> d) & 1u;
        check_shape(shape, flags);
        ++plans;
      }
    }
  }
  unsetenv("OLAP_BLOCKS_BY_STORE");
  // 32 dimensions, alternating: as many merged dimensions as the tables hold
  std::vector<uint32_t> wide(OLAP_MAX_DIMS, 1);
  std::vector<uint8_t> alternating(OLAP_MAX_DIMS);
  for (int d = 0; d < OLAP_MAX_DIMS; ++d) alternating[d] = (uint8_t)(d & 1), wide[d] = d < 14 ? 2 : 1;
  check_shape(wide, alternating);
  for (int d = 0; d < OLAP_MAX_DIMS; ++d) alternating[d] = (uint8_t)(~d & 1);
  check_shape(wide, alternating);
  printf("%d plans checked, %d failures\n", plans + 2, failures);
  return failures ? 1 : 0;
}
