// Stand-alone sanitizer run of the packed fixed-width run printer
// (emit_packed_fixed in csrc/pb2json.hip and csrc/fp_shortest.h, single-lane
// CPU build) through k_pb2json.  The schema is built here by hand: one
// message with `repeated double d = 1`, `repeated float f = 2` and
// `repeated sfixed64 q = 3`.  Every slot gets heap buffers of exactly the
// sizes the engine gives it, so AddressSanitizer sees any read past the wire
// or write past an arena, and UBSan any shift or overflow in the integer
// digit generator.  Cases: mantissa fields 0, 1, all-ones and one
// pseudo-random value at every finite binary exponent of both formats, in
// both signs, in runs of 130 (each double text is also parsed back with
// strtod and compared); then every byte-prefix of a 130-element double run.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -fno-sanitize-recover=undefined -DGGRMCP_HOST_SIM -DWAVE=1 \
//       -Iggrmcp_amd/ops/csrc tools/asan_packed_runs.cpp -o /tmp/asan_packed_runs \
//     && /tmp/asan_packed_runs

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "json2pb.hip"
#include "pb2json.hip"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

static Tables g_tables;
static unsigned g_slots = 0;

// one slot, bare JSON (mode 1); returns the status and the text
static int decode(const std::string& wire, std::string* text) {
  uint32_t len = (uint32_t)wire.size();
  // exact-size heap blocks: one byte past any of them is a finding
  uint8_t* in = (uint8_t*)malloc(len ? len : 1);
  memcpy(in, wire.data(), len);
  uint32_t scap = (len * 8 + 1024 + 15) & ~15u;
  uint32_t fcap = (len * 16 + 2048 + 15) & ~15u;
  uint32_t off[2] = {0, len}, s_off[2] = {0, scap}, f_off[2] = {0, fcap};
  uint8_t* scratch = (uint8_t*)malloc(scap);
  uint8_t* fin = (uint8_t*)malloc(fcap);
  DecodeResult r{};
  int32_t skip = 0, idx = 0;
  threadIdx.x = blockIdx.x = 0;
  k_pb2json(in, off, &idx, nullptr, nullptr, scratch, s_off, fin, f_off, &r,
            &skip, g_tables, 1, 1);
  if (r.status == E_OK) text->assign((const char*)fin + r.out_off, r.out_len);
  free(fin);
  free(scratch);
  free(in);
  ++g_slots;
  return r.status;
}

static std::string run(uint32_t field, const std::string& body) {
  std::string w(1, (char)(field << 3 | 2));
  uint32_t n = (uint32_t)body.size();
  while (n >= 0x80) {
    w.push_back((char)(n | 0x80));
    n >>= 7;
  }
  w.push_back((char)n);
  return w + body;
}

int main() {
  static const char NAMES[] = "dfq";
  MsgEntry msg{0, 3, WKT_NONE, 0};
  FieldEntry fields[3];
  memset(fields, 0, sizeof(fields));
  const uint8_t kinds[3] = {K_DOUBLE, K_FLOAT, K_SFIXED64};
  for (uint32_t i = 0; i < 3; ++i) {
    fields[i].number = i + 1;
    fields[i].name_off = fields[i].json_off = i;
    fields[i].name_len = fields[i].json_len = 1;
    fields[i].sub_index = -1;
    fields[i].kind = kinds[i];
    fields[i].flags = F_REPEATED | F_PACKED;
    fields[i].oneof_id = 255;
  }
  g_tables = Tables{};
  g_tables.msgs = &msg;
  g_tables.fields = fields;
  g_tables.names = (const uint8_t*)NAMES;
  g_tables.n_msgs = 1;
  gridDim.x = 1;

  unsigned values = 0;
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  // every finite binary exponent: width 8 = double, 4 = float
  for (int width = 8; width >= 4; width -= 4) {
    const int mbits = width == 8 ? 52 : 23, n_exp = width == 8 ? 2047 : 255;
    const uint64_t ones = (1ull << mbits) - 1;
    std::vector<uint64_t> bits;
    for (int e = 0; e < n_exp; ++e) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t mant[4] = {0, 1, ones, (lcg >> 11) & ones};
      for (uint64_t m : mant) {
        if (!e && !m) continue;
        uint64_t b = (uint64_t)e << mbits | m;
        bits.push_back(b);
        bits.push_back(b | 1ull << (8 * width - 1));
      }
    }
    for (uint64_t b = 1; b <= 64; ++b) bits.push_back(b);  // first subnormals
    for (size_t at = 0; at < bits.size(); at += 130) {
      size_t n = bits.size() - at < 130 ? bits.size() - at : 130;
      std::string body;
      for (size_t i = 0; i < n; ++i) body.append((const char*)&bits[at + i], width);
      std::string text;
      if (decode(run(width == 8 ? 1 : 2, body), &text) != E_OK) {
        fprintf(stderr, "width %d run at %zu: not E_OK\n", width, at);
        return 1;
      }
      // {"d":[...]} : parse every element back
      const char* p = text.c_str() + 6;
      for (size_t i = 0; i < n; ++i, ++values) {
        char* end;
        double got = strtod(p, &end);
        double want;
        if (width == 8) {
          memcpy(&want, &bits[at + i], 8);
        } else {
          float f;
          uint32_t b32 = (uint32_t)bits[at + i];
          memcpy(&f, &b32, 4);
          want = f;
          got = (float)got;
        }
        if (got != want || (*end != ',' && *end != ']')) {
          fprintf(stderr, "width %d value %zu: %.*s does not parse back\n",
                  width, at + i, (int)(end - p), p);
          return 1;
        }
        p = end + 1;
      }
    }
  }
  // every byte-prefix of a 130-element double run (and of an sfixed64 one):
  // the length prefix always matches the body, so a ragged body is E_PARSE
  unsigned prefixes = 0;
  std::string body;
  for (int i = 0; i < 130; ++i) {
    double v = (i % 7 - 3) * 1.2345678901234567e-7 * (double)(1ull << (i % 60));
    body.append((const char*)&v, 8);
  }
  for (uint32_t field = 1; field <= 3; field += 2) {
    for (size_t n = 0; n <= body.size(); ++n, ++prefixes) {
      std::string text;
      int st = decode(run(field, body.substr(0, n)), &text);
      if (st != (n % 8 ? E_PARSE : E_OK)) {
        fprintf(stderr, "field %u prefix %zu: status %d\n", field, n, st);
        return 1;
      }
    }
  }
  printf("%u values at every binary exponent parsed back, %u run prefixes, "
         "%u slots; no sanitizer report\n", values, prefixes, g_slots);
  return 0;
}
