// Stand-alone sanitizer run of the wire re-ordering pass (reorder_host in
// csrc/pb_reorder.h: k_pb_reorder's own phases, single-lane CPU build) over
// the cases written by reorder_dump.py.  Every slot gets heap buffers of
// exactly the sizes the engine gives it — input, scratch, final, and the
// reorder arena of ro_region — so AddressSanitizer sees any read past the
// input or write past an arena.  The classic kernel runs first, as on the
// device; the pass then sees the slot only when that left E_UNSUPPORTED.
//
//   python tools/reorder_dump.py /tmp/reorder.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc \
//       tools/asan_reorder.cpp -o /tmp/asan_reorder \
//     && /tmp/asan_reorder /tmp/reorder.bin

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "json2pb.hip"
#include "pb2json.hip"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s reorder.bin\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  unsigned total = 0, sections = 0, reordered = 0, redecode_refused = 0,
           gave_up = 0, not_seen = 0;
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
      if (id_len > ID_SLOT_BYTES || !(mode & DM_REORDER)) return 2;
      std::string rid(id_len, '\0');
      if (id_len && !rd(f, &rid[0], id_len)) return 2;
      if (!rd(f, &len, 4)) return 2;
      // exact-size heap blocks: one byte past any of them is a finding
      uint8_t* in = (uint8_t*)malloc(len ? len : 1);
      if (len && !rd(f, in, len)) return 2;
      uint32_t scap = (len * 8 + 1024 + 15) & ~15u;
      uint32_t fcap = ((len * 16 + 2048 + 15) & ~15u) +
                      ((mode & DM_STRUCTURED) ? scap : 0);
      uint32_t off[2] = {0, len}, s_off[2] = {0, scap}, f_off[2] = {0, fcap};
      uint8_t* scratch = (uint8_t*)malloc(scap);
      uint8_t* fin = (uint8_t*)malloc(fcap);
      uint8_t* arena = (uint8_t*)malloc(ro_region(len, 1));
      uint8_t ids[ID_SLOT_BYTES] = {0};
      SlotResult enc{};
      enc.id_len = (uint32_t)rid.size();
      memcpy(ids, rid.data(), rid.size());
      const bool env = (mode & DM_KIND) == 0;
      DecodeResult r{};
      int32_t skip = 0;
      threadIdx.x = blockIdx.x = 0;
      k_pb2json(in, off, &idx, env ? ids : nullptr, env ? &enc : nullptr,
                scratch, s_off, fin, f_off, &r, &skip, t, 1, mode);
      const int classic = r.status;
      reorder_host(in, off, &idx, env ? ids : nullptr, env ? &enc : nullptr,
                   scratch, s_off, fin, f_off, &r, &skip, arena, t, 1, mode);
      if (classic != E_UNSUPPORTED) {
        if (r.status != classic || r.pad != 0) {
          fprintf(stderr, "section %u case %u: a slot at status %d was touched\n",
                  sections, i, classic);
          return 1;
        }
        ++not_seen;
      } else if (r.pad != 3) {
        ++gave_up;
      } else if (r.status != E_OK) {
        ++redecode_refused;
      } else {
        if (r.out_len > fcap) return 1;
        ++reordered;
      }
      free(arena);
      free(fin);
      free(scratch);
      free(in);
    }
  }
  fclose(f);
  printf("%u cases in %u sections: %u reordered and printed, %u refused by "
         "the re-decode, %u given up, %u not E_UNSUPPORTED after k_pb2json; "
         "no sanitizer report\n",
         total, sections, reordered, redecode_refused, gave_up, not_seen);
  return 0;
}
