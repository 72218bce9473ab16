// Stand-alone sanitizer run of the packed varint run printer
// (emit_packed_varint / pv_window in csrc/pb2json.hip, single-lane CPU build)
// through k_pb2json and through the probe's body.  The schema is built here by
// hand: one message with a packed `repeated` field of each of int32, int64,
// uint32, uint64, sint32, sint64, bool and an enum {C_ZERO=0, C_ONE=1,
// C_NEG=-1}.  Every slot gets heap buffers of exactly the sizes named, so
// AddressSanitizer sees any read past the wire (a terminator looked for past
// the run, a fold past the slot) or write past an arena, and UBSan any shift
// or overflow in the fold and the digit code.  Cases: every kind at run
// lengths 1..200 with 1-, 2-, 5- and 10-byte encodings, compared with snprintf;
// non-minimal encodings; 300 ten-byte and 300 one-byte elements; over-long
// varints, unterminated tails and a run that ends inside an element; the
// overflow pair; every byte-prefix of one mixed run per kind.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -fno-sanitize-recover=undefined -DGGRMCP_HOST_SIM -DWAVE=1 \
//       -Iggrmcp_amd/ops/csrc tools/asan_packed_varint.cpp \
//       -o /tmp/asan_packed_varint && /tmp/asan_packed_varint

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
static const uint8_t KINDS[8] = {K_INT32, K_INT64, K_UINT32, K_UINT64,
                                 K_SINT32, K_SINT64, K_BOOL, K_ENUM};

// one slot, bare JSON (mode 1), scratch of `scap` bytes (0: the engine's)
static int decode(const std::string& wire, std::string* text, uint32_t scap = 0) {
  uint32_t len = (uint32_t)wire.size();
  uint8_t* in = (uint8_t*)malloc(len ? len : 1);
  memcpy(in, wire.data(), len);
  if (!scap) scap = (len * 8 + 1024 + 15) & ~15u;
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

static std::string vi(uint64_t v) {
  std::string s;
  for (; v >= 0x80; v >>= 7) s.push_back((char)(v | 0x80));
  s.push_back((char)v);
  return s;
}

static std::string run(uint32_t field, const std::string& body) {
  return vi(field << 3 | 2) + vi(body.size()) + body;
}

// what the decoded varint `v` prints as in field `k` (0..7)
static std::string fmt(int k, uint64_t v) {
  char b[32];
  const int64_t z = (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  switch (KINDS[k]) {
    case K_INT32: snprintf(b, sizeof b, "%d", (int32_t)(uint32_t)v); break;
    case K_INT64: snprintf(b, sizeof b, "\"%lld\"", (long long)v); break;
    case K_UINT32: snprintf(b, sizeof b, "%u", (uint32_t)v); break;
    case K_UINT64: snprintf(b, sizeof b, "\"%llu\"", (unsigned long long)v); break;
    case K_SINT32: snprintf(b, sizeof b, "%d", (int32_t)z); break;
    case K_SINT64: snprintf(b, sizeof b, "\"%lld\"", (long long)z); break;
    case K_BOOL: return v ? "true" : "false";
    default: {
      const int32_t n = (int32_t)(int64_t)v;
      if (n == 0) return "\"C_ZERO\"";
      if (n == 1) return "\"C_ONE\"";
      if (n == -1) return "\"C_NEG\"";
      snprintf(b, sizeof b, "%d", n);
    }
  }
  return b;
}

// wire values of 1, 2, 5 and 10 bytes; every kind reads them its own way
static const uint64_t POOL[] = {0, 1, 2, 127, 128, 300, 16383, 0x7fffffffull,
                                0xffffffffull, 0xfffffffeull, 1ull << 40,
                                ~0ull, ~0ull - 1, 1ull << 63, ~0ull - 8,
                                0xffffffff80000000ull, 9};

static std::string text_of(int k, const std::vector<uint64_t>& vals) {
  std::string t = std::string("{\"") + (char)('a' + k) + "\":[";
  for (size_t i = 0; i < vals.size(); ++i) t += (i ? "," : "") + fmt(k, vals[i]);
  return t + "]}";
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); return 1; } while (0)

int main() {
  static const char NAMES[] = "abcdefghC_ZEROC_ONEC_NEG";
  MsgEntry msg{0, 8, WKT_NONE, 0};
  FieldEntry fields[8];
  memset(fields, 0, sizeof(fields));
  for (uint32_t i = 0; i < 8; ++i) {
    fields[i].number = i + 1;
    fields[i].name_off = fields[i].json_off = i;
    fields[i].name_len = fields[i].json_len = 1;
    fields[i].sub_index = KINDS[i] == K_ENUM ? 0 : -1;
    fields[i].kind = KINDS[i];
    fields[i].flags = F_REPEATED | F_PACKED;
    fields[i].oneof_id = 255;
  }
  EnumEntry en{0, 3};
  EnumValueEntry ev[3];
  memset(ev, 0, sizeof(ev));
  const int32_t nums[3] = {0, 1, -1};
  const uint32_t offs[3] = {8, 14, 19}, lens[3] = {6, 5, 5};
  for (int i = 0; i < 3; ++i) {
    ev[i].number = nums[i];
    ev[i].name_off = offs[i];
    ev[i].name_len = (uint16_t)lens[i];
  }
  g_tables = Tables{};
  g_tables.msgs = &msg;
  g_tables.fields = fields;
  g_tables.enums = &en;
  g_tables.enum_vals = ev;
  g_tables.names = (const uint8_t*)NAMES;
  g_tables.n_msgs = 1;
  gridDim.x = 1;
  const size_t n_pool = sizeof(POOL) / sizeof(POOL[0]);
  std::string text;

  // every kind at every run length, unequal element and text lengths
  unsigned values = 0;
  for (int k = 0; k < 8; ++k) {
    for (size_t n : {1, 2, 63, 64, 65, 128, 129, 200}) {
      std::vector<uint64_t> vals;
      std::string body;
      for (size_t i = 0; i < n; ++i) {
        vals.push_back(POOL[(i * 7 + 3) % n_pool]);
        body += vi(vals.back());
      }
      values += (unsigned)n;
      if (decode(run(k + 1, body), &text) != E_OK || text != text_of(k, vals))
        FAIL("kind %d run of %zu: %s\n", k, n, text.c_str());
    }
  }
  // non-minimal encodings; 300 ten-byte and 300 one-byte elements
  const std::string ones = std::string(9, '\xff') + '\x7f';
  if (decode(run(4, std::string("\x80\x00", 2) + ones), &text) != E_OK ||
      text != text_of(3, {0, ~0ull}))
    FAIL("non-minimal: %s\n", text.c_str());
  for (uint64_t v : {~0ull - 2, 7ull}) {
    std::string body;
    for (int i = 0; i < 300; ++i) body += vi(v);
    if (decode(run(2, body), &text) != E_OK ||
        text != text_of(1, std::vector<uint64_t>(300, v)))
      FAIL("300 x %llu\n", (unsigned long long)v);
  }
  // malformed: an 11-byte varint as element 0, 39 and 49 of 50; a tail of 1..9
  // continuation bytes; a run that ends inside an element whose continuation
  // the next field's bytes would terminate
  const std::string eleven = std::string(10, '\xff') + '\x01';
  for (int at : {0, 39, 49}) {
    std::string body;
    for (int i = 0; i < 50; ++i) body += i == at ? eleven : vi(POOL[i % n_pool]);
    if (decode(run(2, body), &text) != E_PARSE) FAIL("eleven at %d\n", at);
  }
  for (int n = 1; n <= 9; ++n) {
    if (decode(run(2, vi(1) + vi(300) + std::string(n, '\x80')), &text) != E_PARSE)
      FAIL("tail of %d\n", n);
  }
  if (decode(run(2, vi(5) + '\x80') + vi(1 << 3) + vi(1), &text) != E_PARSE)
    FAIL("run ending inside an element\n");
  // overflow: 64 one-digit texts and the longest; scratch to the byte, then
  // the first 64 and ten bytes
  {
    std::vector<uint64_t> vals;
    std::string body;
    for (int i = 0; i < 65; ++i) {
      vals.push_back(i < 64 ? (uint64_t)(i % 10) : 1ull << 63);
      body += vi(vals.back());
    }
    const std::string full = text_of(1, vals);
    if (decode(run(2, body), &text, (uint32_t)full.size()) != E_OK || text != full)
      FAIL("exact scratch\n");
    if (decode(run(2, body), &text, (uint32_t)full.size() - 25 + 10) != E_OVERFLOW)
      FAIL("tight scratch\n");
  }
  // every byte-prefix of a 130-element mixed run per kind: E_OK exactly where
  // the prefix ends on an element boundary; the probe's body too, into a text
  // arena of 4 * prefix bytes
  unsigned prefixes = 0;
  for (int k = 0; k < 8; ++k) {
    std::string body;
    std::vector<bool> boundary(1, true);
    for (int i = 0; i < 130; ++i) {
      const std::string e = vi(POOL[(i * 5 + k) % n_pool]);
      body += e;
      boundary.insert(boundary.end(), e.size() - 1, false);
      boundary.push_back(true);
    }
    for (size_t n = 0; n <= body.size(); ++n, ++prefixes) {
      int st = decode(run(k + 1, body.substr(0, n)), &text);
      if (st != (boundary[n] ? E_OK : E_PARSE))
        FAIL("kind %d prefix %zu: status %d\n", k, n, st);
      if (KINDS[k] == K_ENUM) continue;
      uint8_t* in = (uint8_t*)malloc(n ? n : 1);
      memcpy(in, body.data(), n);
      uint8_t* out = (uint8_t*)malloc(4 * n + 1);
      uint32_t* trace = (uint32_t*)malloc(PV_TRACE_CAP * sizeof(uint32_t));
      uint32_t res[3] = {0, 0, 0};
      pv_probe(in, (uint32_t)n, KINDS[k], out, (uint32_t)(4 * n), trace, res, 0);
      free(trace);
      free(out);
      free(in);
      // a text arena that small may overflow; it may not pass a cut element
      if (!boundary[n] && res[0] == E_OK) FAIL("probe kind %d prefix %zu\n", k, n);
    }
  }
  printf("%u values, %u run prefixes, %u slots; no sanitizer report\n", values,
         prefixes, g_slots);
  return 0;
}
