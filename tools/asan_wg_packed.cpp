// Stand-alone sanitizer run of the packed-run split in the workgroup decode
// kernel's host driver (wgd_scan / wgd_pack_split / wgd_pack_walk in
// csrc/pb2json_wg.h, single-lane CPU build) over the cases written by
// wg_packed_dump.py: the packed-chunk case lists and every byte-prefix of one
// split int64 wire.  Every slot gets heap buffers of exactly the sizes the
// engine gives a routed slot, and the wire an exact-size heap copy, so
// AddressSanitizer sees the boundary search read one byte past a record or a
// chunk's walk write past its region; the classic kernel runs on the same
// slot and (status, bytes) must be equal.
//
//   python tools/wg_packed_dump.py /tmp/wg_packed.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc \
//       tools/asan_wg_packed.cpp -o /tmp/asan_wg_packed \
//     && /tmp/asan_wg_packed /tmp/wg_packed.bin

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

// packed chunks the scanner makes of the slot
static unsigned chunks(const Tables& t, int mode, int32_t idx, const uint8_t* in,
                       uint32_t len) {
  WgDecState* S = new WgDecState;
  WgDecReq q{};
  q.pb = in;
  q.wire_len = len;
  q.msg_idx = idx;
  q.flags = mode & (DM_UNPOPULATED | DM_STRUCTURED);
  threadIdx.x = 0;
  wgd_scan(*S, q, t);
  unsigned n = 0;
  for (int i = 0; S->mode && i < S->nitems; ++i) n += S->pchunk[i] != WGD_PK_NONE;
  delete S;
  return n;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s wg_packed.bin\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  unsigned ok = 0, refused = 0, total = 0, split = 0, n_chunks = 0;
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
      Answer want = run(t, false, mode, idx, in, len, rid, scap_classic,
                        fcap + ((mode & DM_STRUCTURED) ? scap_classic : 0));
      Answer got = run(t, true, mode, idx, in, len, rid, scap,
                       fcap + ((mode & DM_STRUCTURED) ? scap : 0));
      if (got.status != want.status || got.bytes != want.bytes ||
          (got.pad != 1 && got.pad != 2)) {
        fprintf(stderr, "case %u mode %d len %u: classic %d/%zu, workgroup "
                "%d/%zu pad %u\n", i, mode, len, want.status, want.bytes.size(),
                got.status, got.bytes.size(), got.pad);
        return 1;
      }
      unsigned c = chunks(t, mode, idx, in, len);
      split += c != 0;
      n_chunks += c;
      free(in);
      got.status == 0 ? ++ok : ++refused;
    }
  }
  fclose(f);
  printf("%u cases: %u status 0, %u refused; %u with a split run, %u packed "
         "chunks in all; all equal to k_pb2json, no sanitizer report\n",
         total, ok, refused, split, n_chunks);
  return 0;
}
