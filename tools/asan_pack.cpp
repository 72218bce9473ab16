// Stand-alone sanitizer run of k_pack_out's host build (pb2json.hip:
// pack_partial / pack_place / pack_copy through pack_out_host, every one of
// the kernel's 256 thread indices in turn) over the batches of
// tests/test_pack_offsets.py.  The final arena, the packed block and both
// result arrays are heap buffers of exactly the sizes in use, so
// AddressSanitizer sees any read past a slot or write past dst_cap; offsets,
// bytes and the overflow verdict are checked against a plain prefix sum.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc \
//       tools/asan_pack.cpp -o /tmp/asan_pack && /tmp/asan_pack

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "json2pb.hip"
#include "pb2json.hip"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

static unsigned batches = 0, overflowed = 0;

// one batch with real bytes behind every slot; cap: the packed block's size
static bool run(const std::vector<uint32_t>& lens, uint32_t cap) {
  int n = (int)lens.size();
  // arena slots 16-aligned with a gap, as final_cap lays them out
  std::vector<uint32_t> src_off(n + 1);
  uint64_t facc = 0;
  for (int i = 0; i < n; ++i) {
    src_off[i] = (uint32_t)facc;
    facc += ((uint64_t)lens[i] + 15) & ~15ull;
  }
  src_off[n] = (uint32_t)facc;
  uint8_t* fin = (uint8_t*)malloc(facc ? facc : 1);
  for (uint64_t k = 0; k < facc; ++k) fin[k] = (uint8_t)(k * 131 + 7);
  uint8_t* dst = (uint8_t*)malloc(cap ? cap : 1);
  memset(dst, 0xEE, cap ? cap : 1);
  DecodeResult* rs = (DecodeResult*)malloc((n ? n : 1) * sizeof(DecodeResult));
  DecodeResult* packed =
      (DecodeResult*)malloc((n ? n : 1) * sizeof(DecodeResult));
  for (int i = 0; i < n; ++i) rs[i] = {E_OK, src_off[i], lens[i], 0};
  pack_out_host(fin, src_off.data(), rs, dst, packed, cap, n);

  uint64_t acc = 0;
  bool ok = true;
  for (int i = 0; i < n; ++i) acc += ((uint64_t)lens[i] + 3) & ~3ull;
  bool fits = acc <= cap;
  if ((pack_total(packed, n) <= cap) != fits) ok = false;
  if (fits && pack_total(packed, n) != acc) ok = false;
  uint64_t off = 0;
  for (int i = 0; i < n && ok; ++i) {
    if (packed[i].out_len != lens[i] || packed[i].status != E_OK) ok = false;
    if (rs[i].out_off != src_off[i]) ok = false;  // the input stays as it was
    if (fits) {
      if (packed[i].out_off != off) ok = false;
      else if (memcmp(dst + off, fin + src_off[i], lens[i]) != 0) ok = false;
    }
    off += ((uint64_t)lens[i] + 3) & ~3ull;
  }
  if (!fits)  // no slot may have written
    for (uint32_t k = 0; k < cap && ok; ++k)
      if (dst[k] != 0xEE) ok = false;
  ++batches;
  if (!fits) ++overflowed;
  if (!ok)
    fprintf(stderr, "batch of %d, cap %u: wrong offsets or bytes\n", n, cap);
  free(fin);
  free(dst);
  free(rs);
  free(packed);
  return ok;
}

// lengths only (sums past 2^32 have no bytes behind them): nothing may write
static bool run_wrap(const std::vector<uint32_t>& lens) {
  int n = (int)lens.size();
  const uint32_t cap = 64;
  std::vector<uint32_t> src_off(n + 1, 0);
  uint8_t* fin = (uint8_t*)malloc(1);
  uint8_t* dst = (uint8_t*)malloc(cap);
  memset(dst, 0xEE, cap);
  DecodeResult* rs = (DecodeResult*)malloc(n * sizeof(DecodeResult));
  DecodeResult* packed = (DecodeResult*)malloc(n * sizeof(DecodeResult));
  for (int i = 0; i < n; ++i) rs[i] = {E_OK, 0, lens[i], 0};
  pack_out_host(fin, src_off.data(), rs, dst, packed, cap, n);
  bool ok = pack_total(packed, n) > 0xFFFFFFF0ull;
  for (uint32_t k = 0; k < cap; ++k)
    if (dst[k] != 0xEE) ok = false;
  ++batches;
  ++overflowed;
  if (!ok) fprintf(stderr, "wrapping batch of %d reported a small total\n", n);
  free(fin);
  free(dst);
  free(rs);
  free(packed);
  return ok;
}

int main() {
  static const uint32_t L[7] = {0, 1, 3, 4, 5, 1023, 1024};
  static const int N[7] = {1, 2, 255, 256, 257, 513, 4096};
  bool ok = true;
  for (int n : N) {
    for (int shift = 0; shift < 7; ++shift) {
      std::vector<uint32_t> lens(n);
      uint64_t acc = 0;
      for (int i = 0; i < n; ++i) {
        lens[i] = L[(i + shift) % 7];
        acc += ((uint64_t)lens[i] + 3) & ~3ull;
      }
      ok &= run(lens, (uint32_t)acc);                 // total == dst_cap
      if (acc) ok &= run(lens, (uint32_t)acc - 1);    // total == dst_cap + 1
      if (shift == 0) ok &= run(lens, (uint32_t)acc + 4096);
    }
    ok &= run(std::vector<uint32_t>(n, 0), 0);        // all-zero batch
    ok &= run(std::vector<uint32_t>(n, 0), 16);
  }
  ok &= run({5, 3}, 8);
  ok &= run({5, 5}, 15);
  ok &= run_wrap({0x80000000u, 0x80000000u});
  ok &= run_wrap({0xFFFFFFFCu, 4, 4});
  ok &= run_wrap({0xFFFFFFFFu, 1});
  ok &= run_wrap(std::vector<uint32_t>(9, 0x40000000u));
  ok &= run_wrap(std::vector<uint32_t>(4096, 1u << 20));
  ok &= run_wrap(std::vector<uint32_t>(513, 0x7FFFFFFFu));
  if (!ok) return 1;
  printf("%u batches, %u of them past dst_cap: offsets and bytes equal to the "
         "prefix sum, no write past the packed block, no sanitizer report\n",
         batches, overflowed);
  return 0;
}
