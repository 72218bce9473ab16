// Stand-alone sanitizer run of the workgroup decode kernel's host driver
// (wg_decode_host in csrc/pb2json_wg.h: the kernel's own phases, one wave
// index at a time, single-lane CPU build) over the cases written by
// wg_decode_dump.py.  Every slot gets heap buffers of exactly the sizes the
// engine gives a routed slot, so AddressSanitizer sees any read past the
// input or write past an arena, and the classic kernel runs on the same
// slot: (status, bytes) must be equal.  A structured envelope runs twice:
// with the final arena the engine sizes for it (final_cap + scratch_cap), and
// with final_cap alone, where it must end in E_OVERFLOW or the same answer
// and never in a write past the slot.
//
//   python tools/wg_decode_dump.py /tmp/wg_decode.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc \
//       tools/asan_wg_decode.cpp -o /tmp/asan_wg_decode \
//     && /tmp/asan_wg_decode /tmp/wg_decode.bin

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

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

struct Answer {
  int status = 0;
  uint32_t pad = 0;
  std::string bytes;
};

// one slot through the classic kernel (wg false) or the workgroup driver
static Answer run(const Tables& t, bool wg, int mode, int32_t idx,
                  const uint8_t* in, uint32_t len, const std::string& rid,
                  uint32_t scap, uint32_t fcap) {
  uint32_t off[2] = {0, len};
  uint32_t s_off[2] = {0, scap}, f_off[2] = {0, fcap};
  // exact-size heap arenas: one byte past either is a finding
  uint8_t* scratch = (uint8_t*)malloc(scap);
  uint8_t* fin = (uint8_t*)malloc(fcap);
  uint8_t ids[ID_SLOT_BYTES] = {0};
  SlotResult enc{};
  enc.id_len = (uint32_t)rid.size();
  memcpy(ids, rid.data(), rid.size());
  DecodeResult r{};
  int32_t skip = wg ? 2 : 0;
  if (wg)
    wg_decode_host(in, off, &idx, ids, &enc, scratch, s_off, fin, f_off, &r,
                   &skip, t, 1, mode);
  else
    k_pb2json(in, off, &idx, ids, &enc, scratch, s_off, fin, f_off, &r, &skip,
              t, 1, mode);
  Answer a;
  a.status = r.status;
  a.pad = r.pad;
  if (r.status == E_OK) a.bytes.assign((const char*)fin, r.out_len);
  free(scratch);
  free(fin);
  return a;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s wg_decode.bin\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  unsigned ok = 0, refused = 0, total = 0, sections = 0, tight_overflow = 0;
  unsigned items = 0, classic_pass = 0;
  gridDim.x = 1;
  for (;;) {
    std::string blob[7];
    uint32_t n0;
    if (!rd(f, &n0, 4)) break;  // end of file
    for (int b = 0; b < 7; ++b) {
      uint32_t n = n0;
      if (b && !rd(f, &n, 4)) return 2;
      blob[b].resize(n);
      if (n && !rd(f, &blob[b][0], n)) return 2;
    }
    int32_t n_msgs, n_tools;
    uint32_t n_cases;
    if (!rd(f, &n_msgs, 4) || !rd(f, &n_tools, 4) || !rd(f, &n_cases, 4)) return 2;
    Tables t{};
    t.msgs = (const MsgEntry*)blob[0].data();
    t.fields = (const FieldEntry*)blob[1].data();
    t.enums = (const EnumEntry*)blob[2].data();
    t.enum_vals = (const EnumValueEntry*)blob[3].data();
    t.tools = (const ToolEntry*)blob[4].data();
    t.names = (const uint8_t*)blob[5].data();
    t.n_msgs = n_msgs;
    t.n_tools = n_tools;
    t.types = (const TypeEntry*)blob[6].data();
    t.n_types = (int32_t)(blob[6].size() / sizeof(TypeEntry));
    ++sections;
    total += n_cases;
    for (uint32_t i = 0; i < n_cases; ++i) {
      uint8_t mode;
      int32_t idx;
      uint32_t id_len, len;
      if (!rd(f, &mode, 1) || !rd(f, &idx, 4) || !rd(f, &id_len, 4)) return 2;
      if (id_len > ID_SLOT_BYTES || (mode & DM_KIND) != 0) return 2;
      std::string rid(id_len, '\0');
      if (id_len && !rd(f, &rid[0], id_len)) return 2;
      if (!rd(f, &len, 4)) return 2;
      // exact-size heap copy of the input: one byte past it is a finding
      uint8_t* in = (uint8_t*)malloc(len ? len : 1);
      if (len && !rd(f, in, len)) return 2;
      // engine.cpp scratch_cap / final_cap for a routed slot
      uint32_t scap_classic = (len * 8 + 1024 + 15) & ~15u;
      uint32_t scap = (len * 8 + 1024 + WG_DEC_EXTRA +
                       ((mode & DM_UNPOPULATED) ? WG_DEC_FILL : 0) + 15) & ~15u;
      uint32_t fcap = (len * 16 + 2048 + 15) & ~15u;
      uint32_t fext = (mode & DM_STRUCTURED) ? scap : 0;
      Answer want = run(t, false, mode, idx, in, len, rid, scap_classic,
                        fcap + ((mode & DM_STRUCTURED) ? scap_classic : 0));
      Answer got = run(t, true, mode, idx, in, len, rid, scap, fcap + fext);
      if (got.status != want.status || got.bytes != want.bytes ||
          (got.pad != 1 && got.pad != 2)) {
        fprintf(stderr, "section %u case %u mode %d: classic %d/%zu, "
                "workgroup %d/%zu pad %u\n", sections, i, mode, want.status,
                want.bytes.size(), got.status, got.bytes.size(), got.pad);
        return 1;
      }
      if (mode & DM_STRUCTURED) {
        Answer tight = run(t, true, mode, idx, in, len, rid, scap, fcap);
        if (got.status == 0 && tight.status == E_OVERFLOW) ++tight_overflow;
        else if (tight.status != got.status || tight.bytes != got.bytes) {
          fprintf(stderr, "section %u case %u: status %d, tight arena %d\n",
                  sections, i, got.status, tight.status);
          return 1;
        }
      }
      free(in);
      got.status == 0 ? ++ok : ++refused;
      got.pad == 1 ? ++items : ++classic_pass;
    }
  }
  fclose(f);
  printf("%u cases in %u sections: %u status 0, %u refused; %u by the item "
         "walk, %u by the in-block classic pass; %u overflowed the unextended "
         "final arena; all equal to k_pb2json, no sanitizer report\n",
         total, sections, ok, refused, items, classic_pass, tight_overflow);
  return 0;
}
