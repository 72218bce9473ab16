// Stand-alone sanitizer run of the kernel logic (single-lane CPU build, see
// csrc/host_shim.h) over the protojson corpus written by corpus_dump.py.
// Every slot gets heap buffers of exactly the sizes the engine gives it
// (engine/hostsim.py), so AddressSanitizer sees any read past the input or
// write past an arena; a watchdog count bounds each slot's output instead.
//
//   python tools/corpus_dump.py /tmp/corpus.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc tools/asan_corpus.cpp \
//       -o /tmp/asan_corpus && /tmp/asan_corpus /tmp/corpus.bin

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

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  unsigned ok = 0, refused = 0, total = 0, sections = 0;
  gridDim.x = 1;
  // one section per schema (corpus_dump.py): 7 table blobs, counts, cases
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
      uint8_t dir;
      int32_t idx;
      uint32_t len;
      if (!rd(f, &dir, 1) || !rd(f, &idx, 4) || !rd(f, &len, 4)) return 2;
      // exact-size heap copy of the input: one byte past it is a finding
      uint8_t* in = (uint8_t*)malloc(len ? len : 1);
      if (len && !rd(f, in, len)) return 2;
      uint32_t off[2] = {0, len};
      int status;
      if (dir == 0) {
        uint32_t cap = (len + len / 4 + 192 + 15) & ~15u;
        uint32_t pb_off[2] = {0, cap};
        std::vector<uint8_t> pb(cap), ids(ID_SLOT_BYTES);
        SlotResult r{};
        Limits lim{10, 1024, 1u << 20, 0};
        k_json2pb(in, off, pb.data(), pb_off, &r, ids.data(), &idx, t, lim, 1, 1,
                  nullptr);
        status = r.status;
      } else {
        uint32_t scap = (len * 8 + 1024 + 15) & ~15u, fcap = (len * 16 + 2048 + 15) & ~15u;
        uint32_t s_off[2] = {0, scap}, f_off[2] = {0, fcap};
        std::vector<uint8_t> scratch(scap), fin(fcap);
        DecodeResult r{};
        k_pb2json(in, off, &idx, nullptr, nullptr, scratch.data(), s_off, fin.data(),
                  f_off, &r, nullptr, t, 1, 1);
        status = r.status;
      }
      free(in);
      status == 0 ? ++ok : ++refused;
    }
  }
  fclose(f);
  printf("%u cases in %u sections: %u status 0, %u refused, no sanitizer report\n",
         total, sections, ok, refused);
  return 0;
}
