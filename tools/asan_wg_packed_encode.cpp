// Stand-alone sanitizer run of the packed-array chunk items of k_json2pb_wg
// (wg_pack_chunk, encode_packed_run and wg_pack_backfill in csrc/json2pb.hip,
// single-lane CPU build) through wg_pack_chunks_host, which gives every chunk
// a heap copy of exactly its text and a heap item of exactly the kernel's
// capacity.  The schema is built here by hand: one message with a repeated
// field of each of double, float, int32, sint64, uint64, fixed32, bool and an
// enum {A = 0, B = 1, N = -1}.  Cases: for every kind a 200-element array
// (and one of about 9 KB, as the device tests use) cut at 0, 1, 2 and 7
// commas, each equal to k_json2pb's record for the whole array; every comma
// of a 200-element double, int32 and enum array as the single cut; the
// refused chunk texts of tests/test_wg_packed_encode_host.py; chunk overflow;
// the backfill helper at and past LEN_SLOT_MAX.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -fno-sanitize-recover=undefined -DGGRMCP_HOST_SIM -DWAVE=1 \
//       -Iggrmcp_amd/ops/csrc tools/asan_wg_packed_encode.cpp \
//       -o /tmp/asan_wg_packed_encode && /tmp/asan_wg_packed_encode

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "json2pb.hip"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

static Tables g_tables;
static unsigned g_runs = 0;
static const int N_KINDS = 8;
static const char NAMES[] = "dfistxbeABN";  // field i is NAMES[i]; enum names

// the whole array through k_json2pb, bare message (mode 1)
static int whole(int field, const std::string& elems, std::string* wire) {
  std::string doc = std::string("{\"") + NAMES[field] + "\":[" + elems + "]}";
  uint32_t len = (uint32_t)doc.size();
  uint32_t cap = (len + len / 4 + 192 + 15) & ~15u;
  uint8_t* in = (uint8_t*)malloc(len);
  memcpy(in, doc.data(), len);
  uint8_t* pb = (uint8_t*)malloc(cap);
  uint8_t ids[ID_SLOT_BYTES];
  uint32_t in_off[2] = {0, len}, pb_off[2] = {0, cap};
  int32_t mi = 0;
  SlotResult r{};
  Limits lim{10, 1024, 1u << 20, 0};
  threadIdx.x = blockIdx.x = 0;
  k_json2pb(in, in_off, pb, pb_off, &r, ids, &mi, g_tables, lim, 1, 1, nullptr);
  if (r.status == E_OK) wire->assign((const char*)pb + r.pb_off, r.pb_len);
  free(pb);
  free(in);
  return r.status;
}

static int cut(int field, const std::string& elems,
               const std::vector<uint32_t>& cuts, std::string* wire) {
  ++g_runs;
  // exact-size heap copy of the text: a read past it is a finding
  uint8_t* text = (uint8_t*)malloc(elems.size() ? elems.size() : 1);
  memcpy(text, elems.data(), elems.size());
  int st = wg_pack_chunks_host(g_tables, field, text, (uint32_t)elems.size(),
                               cuts.data(), (int)cuts.size(), wire);
  free(text);
  return st;
}

static std::string element(int field, unsigned i) {
  char b[64];
  switch (field) {
    case 0: snprintf(b, sizeof b, "%.17g", i * 0.37 + 0.001); break;
    case 1: snprintf(b, sizeof b, "%g", i * 0.25 + 0.125); break;
    case 2: snprintf(b, sizeof b, "%u", i % 10); break;
    case 3: snprintf(b, sizeof b, "-%u", i * 7919u + 1); break;
    case 4: snprintf(b, sizeof b, "%" PRIu64, (uint64_t)(1ull << 40) + i); break;
    case 5: snprintf(b, sizeof b, "%u", i * 65537u); break;
    case 6: snprintf(b, sizeof b, "%s", i % 3 ? "true" : "false"); break;
    default: {
      // few negatives: ten bytes of wire each, and an item holds 5/4 of its text
      static const char* E[9] = {"\"B\"", "1", "\"A\"", "0", "\"B\"", "1",
                                 "\"N\"", "0", "-1"};
      snprintf(b, sizeof b, "%s", E[i % 9]);
    }
  }
  if (field < 6 && i % 5 == 2) return std::string("\"") + b + "\"";
  if (field < 2 && i % 50 == 7) return "\"NaN\"";
  return b;
}

static std::string array_text(int field, size_t n_elems, size_t n_bytes) {
  std::string s;
  for (unsigned i = 0; i < n_elems || s.size() < n_bytes; ++i) {
    if (i) s += i % 11 == 3 ? " ,\n" : ",";
    s += element(field, i);
  }
  return s;
}

static std::vector<uint32_t> commas(const std::string& s) {
  std::vector<uint32_t> v;
  for (uint32_t i = 0; i < s.size(); ++i)
    if (s[i] == ',') v.push_back(i);
  return v;
}

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

int main() {
  MsgEntry msg{0, N_KINDS, WKT_NONE, 0};
  FieldEntry fields[N_KINDS];
  memset(fields, 0, sizeof(fields));
  const uint8_t kinds[N_KINDS] = {K_DOUBLE, K_FLOAT, K_INT32, K_SINT64,
                                  K_UINT64, K_FIXED32, K_BOOL, K_ENUM};
  for (uint32_t i = 0; i < N_KINDS; ++i) {
    FieldEntry& f = fields[i];
    f.number = i < 4 ? i + 1 : 3000 + i;  // one- and two-byte tags
    f.name_off = f.json_off = i;
    f.name_len = f.json_len = 1;
    f.hash_json = f.hash_orig = fnv1a64((const uint8_t*)NAMES + i, 1);
    f.sub_index = kinds[i] == K_ENUM ? 0 : -1;
    f.kind = kinds[i];
    f.flags = F_REPEATED | F_PACKED;
    f.oneof_id = 255;
  }
  EnumEntry en{0, 3};
  EnumValueEntry ev[3];
  memset(ev, 0, sizeof(ev));
  const int32_t numbers[3] = {0, 1, -1};
  for (uint32_t i = 0; i < 3; ++i) {
    ev[i].name_off = N_KINDS + i;
    ev[i].name_len = 1;
    ev[i].hash = fnv1a64((const uint8_t*)NAMES + N_KINDS + i, 1);
    ev[i].number = numbers[i];
  }
  g_tables = Tables{};
  g_tables.msgs = &msg;
  g_tables.fields = fields;
  g_tables.enums = &en;
  g_tables.enum_vals = ev;
  g_tables.names = (const uint8_t*)NAMES;
  g_tables.n_msgs = 1;
  gridDim.x = 1;

  // cut arrays equal the whole array's record
  static const int CUTS[4] = {0, 1, 2, 7};
  for (int field = 0; field < N_KINDS; ++field) {
    for (int big = 0; big < 2; ++big) {
      std::string text = array_text(field, 200, big ? 9300 : 0), want, got;
      CHECK(whole(field, text, &want) == E_OK, "field %d: whole array refused", field);
      std::vector<uint32_t> cm = commas(text);
      for (int n : CUTS) {
        std::vector<uint32_t> cuts;
        for (int k = 0; k < n; ++k) cuts.push_back(cm[(k + 1) * cm.size() / (n + 1)]);
        CHECK(cut(field, text, cuts, &got) == E_OK && got == want,
              "field %d, %d cuts: differs from the whole array", field, n);
      }
      if (big || (field != 0 && field != 2 && field != 7)) continue;
      for (uint32_t at : cm)  // every comma as the single cut
        CHECK(cut(field, text, {at}, &got) == E_OK && got == want,
              "field %d cut at %u: differs from the whole array", field, at);
    }
  }

  // doubles only the window converts, each the last element of its chunk
  {
    std::string text = "5e-324,1.7976931348623157e308,2.2250738585072014e-308,"
                       "0.1000000000000000055511151231257827", want, got;
    CHECK(whole(0, text, &want) == E_OK, "extreme doubles: whole array refused");
    CHECK(cut(0, text, commas(text), &got) == E_OK && got == want,
          "extreme doubles, one per chunk: differs from the whole array");
  }

  // refused chunks: int32 through the window, enum through the serial loop
  struct Bad { const char* text; std::vector<uint32_t> cuts; };
  const Bad bad[] = {
      {"1,,2", {1, 2}}, {"1,2,", {3}}, {",1,2", {0}}, {"1, \t,2", {1, 4}},
      {"1,2,,3", {1}},  {"1,2,", {1}}, {"1,2],[3,4", {4}}, {"1,2]", {}},
      {"1,2 x", {1}},   {"", {}},      {" ", {}}};
  for (const Bad& b : bad)
    for (int field : {2, 7}) {
      std::string got;
      CHECK(cut(field, b.text, b.cuts, &got) > 0 && got.empty(),
            "field %d: \"%s\" was not refused", field, b.text);
    }

  // 8 bytes of wire for 2 of text: the item is full before the chunk ends
  std::string zeros = "0", got;
  for (int i = 1; i < 100; ++i) zeros += ",0";
  CHECK(cut(0, zeros, {}, &got) == E_OVERFLOW, "double zeros: no E_OVERFLOW");
  CHECK(cut(0, zeros, {99}, &got) == E_OVERFLOW, "double zeros, cut: no E_OVERFLOW");
  CHECK(cut(2, zeros, {99}, &got) == E_OK, "int32 zeros refused");

  // the backfill at and past LEN_SLOT_MAX (lengths only: the item is 8 bytes)
  std::vector<uint32_t> lens(512, 4096);
  lens[0] += 1 + LEN_SLOT;
  lens[511] = 4095;
  uint8_t* item = (uint8_t*)malloc(1 + LEN_SLOT);
  CHECK(wg_pack_backfill(item, 1, lens.data(), 512) && item[1] == 0xFF &&
            item[2] == 0xFF && item[3] == 0x7F,
        "backfill at LEN_SLOT_MAX");
  lens[511] = 4096;
  CHECK(!wg_pack_backfill(item, 1, lens.data(), 512), "backfill past LEN_SLOT_MAX");
  free(item);

  printf("%u chunked encodes; no sanitizer report\n", g_runs);
  return 0;
}
