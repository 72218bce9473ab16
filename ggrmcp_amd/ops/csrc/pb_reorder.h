// k_pb_reorder — canonical re-ordering of protobuf wire on the device
// (gfx950, wave64), included at the end of pb2json.hip.
//
// The single-pass decode walkers print a body only when its known fields
// arrive in ascending field number.  The wire format promises no order, and
// a re-occurring field is a merge.  With DM_REORDER this pass runs after the
// decode kernels: one wave per slot they left at E_UNSUPPORTED rewrites the
// slot's wire into canonical order (the protobuf merge of the message) in a
// separate arena, then decodes that with the classic walker.  A slot the
// pass cannot serve keeps its DecodeResult untouched, so the host answers it
// as before.
//
// reorder_walk is an iterative depth-first walk with an explicit frame
// stack.  Per body (message index + source byte range):
//   index   serial tag scan -> run records in the wave's LDS window;
//           adjacent occurrences of one field collapse into one run
//   select  protobuf merge rules, one record per lane against the window
//   sort    stable rank by (field number, arrival), 64 records per step,
//           keys in registers; survivors scatter to the wave's record
//           stack in global memory, where they outlive the children's use
//           of the window
//   emit    plain runs: lengths -> offsets by a wave scan, verbatim copies;
//           message occurrences: tag, LEN_SLOT-wide length slot (backfilled
//           at pop), child frame
// Phases are DEV/DEVN functions over RoState, so the CPU build drives the
// same code at WAVE=1.  Control flow is wave-uniform; lanes are a parallel
// unit only inside select, sort, the scan and the copies.
#pragma once

// one run of a body: occurrences [start, end) of field-table entry fidx
struct RoRec {
  uint32_t fidx, start, end, count;
};
static_assert(sizeof(RoRec) == 16, "RoRec layout");

struct RoFrame {
  const uint8_t* src;  // the body's bytes (slot wire or side buffer)
  uint32_t rec_base;   // its sorted records in the wave's record stack
  uint32_t rec_n;
  uint32_t cur;        // next record to emit
  uint32_t occ;        // resume offset inside a message run (0: at its start)
  uint32_t slot;       // output offset of its length slot (RO_NO_SLOT: top)
  uint32_t side_save;  // side-buffer top to restore when it pops
};
constexpr uint32_t RO_NO_SLOT = 0xFFFFFFFFu;

// meta word of a window record
enum : uint32_t {
  ROM_ONEOF = 0xFF,     // oneof id (255 = none)
  ROM_SINGULAR = 0x100, // singular non-message field: last occurrence wins
  ROM_ALIVE = 0x200,    // survived select
};

// the wave's LDS window: run records as arrays (a lane reads one column of
// its own record, all lanes read record j for a compare) + the frame stack
struct RoWin {
  uint32_t fidx[RO_MAX_RUNS], num[RO_MAX_RUNS], start[RO_MAX_RUNS],
      end[RO_MAX_RUNS], count[RO_MAX_RUNS], last[RO_MAX_RUNS],
      meta[RO_MAX_RUNS];
  RoFrame frames[MAX_RECURSE];
};

struct RoState {
  RoWin* win;
  RoRec* stack;  // RO_STACK_RUNS records, owned by the wave in flight
  uint8_t* out;  // canonical wire
  uint32_t out_cap, opos;
  uint8_t* side;  // merged singular-message payloads, stack discipline
  uint32_t side_cap, side_top;
  uint32_t rec_top;
  int sp;
  int lane;
  Tables t;
};

// writes of one lane read by another lane of the same wave go through memory
DEV void ro_fence() {
#ifndef GGRMCP_HOST_SIM
  __threadfence_block();
#endif
}

DEV void ro_copy(uint8_t* dst, const uint8_t* src, uint32_t n, int lane) {
  for (uint32_t i = (uint32_t)lane; i < n; i += WAVE) dst[i] = src[i];
}

DEV uint32_t ro_varint_size(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

// ---- index ------------------------------------------------------------------
// Tag scan of src[0, len) as message msg_idx: read_tag and skip_wire give the
// classic walker's own malformed-wire checks.  Unknown fields, unknown groups
// and known numbers in a foreign wire type produce no record and end the
// open run (the canonical wire drops them).  false = give up.
DEVN bool ro_index(RoState& S, const uint8_t* src, uint32_t len, int msg_idx,
                   uint32_t* n_out) {
  DCtx c;
  wgd_ctx(c, S.t, nullptr, 0);
  c.pb = src;
  c.len = len;
  RoWin& w = *S.win;
  const MsgEntry& m = S.t.msgs[msg_idx];
  uint32_t n = 0;
  bool open = false;  // record n-1 may still take adjacent occurrences
  while (c.pos < len) {
    uint32_t occ = c.pos;
    uint64_t tag;
    if (!read_tag(c, &tag)) return false;
    uint32_t num = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    const FieldEntry* fe = find_field(c, m, num);
    if (fe && fe->kind == K_GROUP) return false;
    if (!skip_wire(c, wt, num)) return false;
    if (!fe ||
        (wt != expected_wire(*fe) && !((fe->flags & F_REPEATED) && wt == W_LEN))) {
      open = false;
      continue;
    }
    uint32_t fidx = (uint32_t)(fe - S.t.fields);
    if (open && w.fidx[n - 1] == fidx) {
      w.end[n - 1] = c.pos;
      w.count[n - 1] += 1;
      w.last[n - 1] = occ;
      continue;
    }
    if (n == (uint32_t)RO_MAX_RUNS) return false;
    // oneof ids saturate in the table compiler: two oneofs may share the
    // last id, and select could not tell their members apart
    if ((fe->flags & F_ONEOF) && fe->oneof_id >= 254) return false;
    w.fidx[n] = fidx;
    w.num[n] = num;
    w.start[n] = occ;
    w.end[n] = c.pos;
    w.count[n] = 1;
    w.last[n] = occ;
    w.meta[n] =
        ((fe->flags & F_ONEOF) ? (uint32_t)fe->oneof_id : 255u) |
        (!(fe->flags & F_REPEATED) && fe->kind != K_MESSAGE ? ROM_SINGULAR : 0u);
    ++n;
    open = true;
  }
  *n_out = n;
  return true;
}

// ---- select + sort ----------------------------------------------------------
// Lane l judges record base+l against the whole window (records j read at a
// wave-uniform index).  A record dies when a later run of the same singular
// field exists (last wins), or a later run of ANOTHER member of its oneof
// (X1 Y X2 -> X2; X1 X2 -> both).  A surviving singular run is cut to its
// last occurrence.  Then each survivor's rank among the survivors by
// (number, arrival) is its place on the record stack: a counting rank needs
// no exchange steps, reads the window once per 64 records and is stable by
// construction.  false = the record stack would overflow.
DEVN bool ro_select_sort(RoState& S, uint32_t n, uint32_t* n_alive) {
  RoWin& w = *S.win;
  uint32_t alive = 0;
  for (uint32_t base = 0; base < n; base += WAVE) {
    uint32_t r = base + (uint32_t)S.lane;
    bool valid = r < n;
    uint32_t rr = valid ? r : 0;
    uint32_t myf = w.fidx[rr], mym = w.meta[rr];
    uint32_t myo = mym & ROM_ONEOF;
    bool dead = false;
    for (uint32_t j = base + 1; j < n; ++j) {
      uint32_t fj = w.fidx[j], oj = w.meta[j] & ROM_ONEOF;
      bool later = j > r;
      if (later && (mym & ROM_SINGULAR) && fj == myf) dead = true;
      if (later && myo != 255u && oj == myo && fj != myf) dead = true;
    }
    if (valid) {
      w.meta[r] = (mym & ~ROM_ALIVE) | (dead ? 0u : ROM_ALIVE);
      if (mym & ROM_SINGULAR) {
        w.start[r] = w.last[r];
        w.count[r] = 1;
      }
    }
    uint64_t am = __ballot(valid && !dead);
    for (; am; am &= am - 1) ++alive;
  }
  if (S.rec_top + alive > (uint32_t)RO_STACK_RUNS) return false;
  for (uint32_t base = 0; base < n; base += WAVE) {
    uint32_t r = base + (uint32_t)S.lane;
    bool valid = r < n;
    uint32_t rr = valid ? r : 0;
    uint32_t key = w.num[rr];
    bool mine = valid && (w.meta[rr] & ROM_ALIVE);
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {
      uint32_t kj = w.num[j];
      bool aj = (w.meta[j] & ROM_ALIVE) != 0;
      if (aj && (kj < key || (kj == key && j < r))) ++rank;
    }
    if (mine) {
      RoRec rec;
      rec.fidx = w.fidx[r];
      rec.start = w.start[r];
      rec.end = w.end[r];
      rec.count = w.count[r];
      S.stack[S.rec_top + rank] = rec;
    }
  }
  ro_fence();
  *n_alive = alive;
  return true;
}

// index, select and sort one body and push its frame.  false = give up.
DEVN bool ro_push(RoState& S, const uint8_t* src, uint32_t len, int msg_idx,
                  uint32_t slot, uint32_t side_save) {
  if (S.sp >= MAX_RECURSE) return false;
  uint32_t n = 0, alive = 0;
  if (!ro_index(S, src, len, msg_idx, &n)) return false;
  if (!ro_select_sort(S, n, &alive)) return false;
  RoFrame& f = S.win->frames[S.sp++];
  f.src = src;
  f.rec_base = S.rec_top;
  f.rec_n = alive;
  f.cur = 0;
  f.occ = 0;
  f.slot = slot;
  f.side_save = side_save;
  S.rec_top += alive;
  return true;
}

// ---- emit -------------------------------------------------------------------
// Copy the non-message runs that lead f's remaining records, up to WAVE per
// step: lane l loads record cur+l, an inclusive wave scan of the lengths
// gives every run its output offset, then the wave copies the whole stretch.
// Stops in front of a message run (or at the end of the records).
DEVN bool ro_emit_plain(RoState& S, RoFrame& f) {
  while (f.cur < f.rec_n) {
    uint32_t left = f.rec_n - f.cur;
    uint32_t batch = left < (uint32_t)WAVE ? left : (uint32_t)WAVE;
    bool valid = (uint32_t)S.lane < batch;
    RoRec r = S.stack[f.rec_base + f.cur + (valid ? (uint32_t)S.lane : 0u)];
    bool is_msg = valid && S.t.fields[r.fidx].kind == K_MESSAGE;
    uint64_t mm = __ballot(is_msg);
    uint32_t m = mm ? (uint32_t)__ffsll((long long)mm) - 1u : batch;
    if (m == 0) return true;
    uint32_t mylen = (uint32_t)S.lane < m ? r.end - r.start : 0u;
    uint32_t incl = mylen;
    for (int d = 1; d < WAVE; d <<= 1) {
      uint32_t up = __shfl_up(incl, d, WAVE);
      if (S.lane >= d) incl += up;
    }
    uint32_t total = __shfl(incl, (int)m - 1, WAVE);
    if (total > S.out_cap - S.opos) return false;
    uint32_t excl = incl - mylen;
    // lanes span the CONCATENATED output (runs are a few bytes each): lane
    // byte i belongs to run k = #{incl <= i}, found by a binary search over
    // the lanes' scan values
    for (uint32_t base = 0; base < total; base += WAVE) {
      uint32_t i = base + (uint32_t)S.lane;
      uint32_t k = 0;
      for (uint32_t w = WAVE / 2; w; w >>= 1) {
        uint32_t probe = k + w - 1;
        uint32_t pv = __shfl(incl, (int)(probe < (uint32_t)WAVE ? probe : 0u), WAVE);
        if (k + w <= m && pv <= i) k += w;
      }
      uint32_t s = __shfl(r.start, (int)k, WAVE);
      uint32_t o = __shfl(excl, (int)k, WAVE);
      if (i < total) S.out[S.opos + i] = f.src[s + (i - o)];
    }
    S.opos += total;
    f.cur += m;
    if (mm) return true;
  }
  return true;
}

// one length-delimited occurrence at src[pos, end): payload offset, length,
// and where the next occurrence starts
DEV bool ro_occ(const uint8_t* src, uint32_t pos, uint32_t end, uint32_t* p,
                uint32_t* len, uint32_t* next) {
  uint64_t tag, v;
  if (!get_varint(src, end, &pos, &tag)) return false;
  if (!get_varint(src, end, &pos, &v)) return false;
  if (v > end - pos) return false;
  *p = pos;
  *len = (uint32_t)v;
  *next = pos + (uint32_t)v;
  return true;
}

// Rewrite wire[0, len) as message top_msg into S.out in canonical order.
// false = give up (S.out holds garbage).  Every loop is bounded: ro_index's
// cursor only moves forward, records and occurrences are counted, and each
// push consumes a strictly shorter body or one of at most MAX_RECURSE levels.
DEV bool reorder_walk(RoState& S, const uint8_t* wire, uint32_t len,
                      int top_msg) {
  S.opos = 0;
  S.side_top = 0;
  S.rec_top = 0;
  S.sp = 0;
  if (!ro_push(S, wire, len, top_msg, RO_NO_SLOT, 0)) return false;
  while (S.sp > 0) {
    RoFrame& f = S.win->frames[S.sp - 1];
    if (f.occ == 0 && !ro_emit_plain(S, f)) return false;
    if (f.cur >= f.rec_n) {
      if (f.slot != RO_NO_SLOT) {
        uint32_t clen = S.opos - (f.slot + LEN_SLOT);
        if (clen > LEN_SLOT_MAX) return false;
        if (!S.lane) put_varint_fixed(S.out + f.slot, clen, LEN_SLOT);
      }
      S.side_top = f.side_save;
      S.rec_top = f.rec_base;
      --S.sp;
      continue;
    }
    // record f.cur is message-typed: a singular message, a repeated message
    // element or a map entry
    RoRec r = S.stack[f.rec_base + f.cur];
    const FieldEntry& fe = S.t.fields[r.fidx];
    const uint8_t* csrc;
    uint32_t clen;
    uint32_t side_save = S.side_top;
    if (!(fe.flags & F_REPEATED)) {
      // every surviving occurrence merges into ONE child body; the runs of
      // one field are adjacent after the sort
      uint32_t g = 0, occs = 0;
      while (f.cur + g < f.rec_n &&
             S.stack[f.rec_base + f.cur + g].fidx == r.fidx) {
        occs += S.stack[f.rec_base + f.cur + g].count;
        ++g;
      }
      if (occs == 1) {
        uint32_t p, next;
        if (!ro_occ(f.src, r.start, r.end, &p, &clen, &next)) return false;
        csrc = f.src + p;
      } else {
        for (uint32_t k = 0; k < g; ++k) {
          RoRec rk = S.stack[f.rec_base + f.cur + k];
          uint32_t pos = rk.start;
          for (uint32_t i = 0; i < rk.count; ++i) {
            uint32_t p, l, next;
            if (!ro_occ(f.src, pos, rk.end, &p, &l, &next)) return false;
            if (l > S.side_cap - S.side_top) return false;
            ro_copy(S.side + S.side_top, f.src + p, l, S.lane);
            S.side_top += l;
            pos = next;
          }
        }
        ro_fence();
        csrc = S.side + side_save;
        clen = S.side_top - side_save;
      }
      f.cur += g;
    } else {
      uint32_t p, next;
      if (!ro_occ(f.src, f.occ ? f.occ : r.start, r.end, &p, &clen, &next))
        return false;
      if (next >= r.end) {
        f.cur += 1;
        f.occ = 0;
      } else {
        f.occ = next;
      }
      csrc = f.src + p;
    }
    if (clen > LEN_SLOT_MAX) return false;
    uint64_t tag = ((uint64_t)fe.number << 3) | W_LEN;
    uint32_t tlen = ro_varint_size(tag);
    if (tlen + LEN_SLOT > S.out_cap - S.opos) return false;
    if (!S.lane) put_varint(S.out + S.opos, tag);
    S.opos += tlen;
    uint32_t slot = S.opos;
    S.opos += LEN_SLOT;
    if (!ro_push(S, csrc, clen, fe.sub_index, slot, side_save)) return false;
  }
  ro_fence();
  return true;
}

// ---- re-decode --------------------------------------------------------------
// k_pb2json's per-slot body over the canonical wire, with the slot's own mode
// bits, into the slot's own scratch and final regions (a copy of that thin
// glue, so the other kernels' resource lines stay where they are).
static __device__ const char RO_C1[] = "{\"type\":\"text\",\"text\":\"";
static __device__ const char RO_C2[] = "\"}";

struct RoReq {
  const uint8_t* pb;  // the slot's delivered wire
  uint32_t wire_len;
  uint8_t* scr;
  uint32_t scr_cap;
  uint8_t* fout;
  uint32_t fcap;
  int msg_idx;
  const uint8_t* idp;
  uint32_t idl;
};

DEV void ro_redecode(RoState& S, const RoReq& q, int mode, DecodeResult* result,
                     uint32_t out_off) {
  const int lane = S.lane;
  const int kind = mode & DM_KIND;
  DecodeResult r;
  r.status = E_OK;
  r.out_off = out_off;
  r.out_len = 0;
  r.pad = 3;
  DCtx c;
  wgd_ctx(c, S.t, q.scr, q.scr_cap);
  c.pb = S.out;
  c.len = S.opos;
  c.unpop = kind != 2 ? (uint32_t)(mode & DM_UNPOPULATED) : 0u;
  decode_walk(c, q.msg_idx, c.len);
  if (c.status != E_OK) {
    r.status = c.status;
    if (!lane) *result = r;
    return;
  }
  uint32_t json_len = c.opos;
  DCtx o;
  wgd_ctx(o, S.t, q.fout, q.fcap);
  bool ok = true;
  if (kind == 1) {
    if (json_len > o.ocap) ok = dfail(o, E_OVERFLOW);
    if (ok) {
      ro_copy(o.out, q.scr, json_len, lane);
      o.opos = json_len;
    }
  } else if (kind == 2) {
    ok = puts_(o, RO_C1, sizeof(RO_C1) - 1);
    if (ok) ok = put_escaped(o, q.scr, json_len);
    if (ok) ok = puts_(o, RO_C2, sizeof(RO_C2) - 1);
  } else {
    ok = puts_(o, WG_P1, sizeof(WG_P1) - 1);
    if (ok && q.idl) {
      if (o.opos + q.idl > o.ocap) ok = dfail(o, E_OVERFLOW);
      if (ok) {
        ro_copy(o.out + o.opos, q.idp, q.idl, lane);
        o.opos += q.idl;
      }
    } else if (ok) {
      ok = puts_(o, "null", 4);
    }
    if (ok) ok = puts_(o, WG_P2, sizeof(WG_P2) - 1);
    if (ok) ok = put_escaped(o, q.scr, json_len);
    if (ok && (mode & DM_STRUCTURED)) {
      ok = puts_(o, WG_S1, sizeof(WG_S1) - 1);
      if (ok && o.opos + json_len > o.ocap) ok = dfail(o, E_OVERFLOW);
      if (ok) {
        ro_copy(o.out + o.opos, q.scr, json_len, lane);
        o.opos += json_len;
        ok = puts_(o, WG_S2, sizeof(WG_S2) - 1);
      }
    } else if (ok) {
      ok = puts_(o, WG_P3, sizeof(WG_P3) - 1);
    }
  }
  if (!ok) r.status = o.status;
  else r.out_len = o.opos;
  if (!lane) *result = r;
}

// Where a slot's canonical wire and side buffer live in the reorder arena,
// from its response offset and batch index alone: 2*len + RO_SLOT_PAD bytes
// of wire (every message occurrence may grow by LEN_SLOT - 1), then len bytes
// of side buffer.  The arena holds 3 * (response bytes) + RO_SLOT_PAD * slots.
DEV size_t ro_region(uint32_t resp_off, int slot) {
  return 3 * (size_t)resp_off + (size_t)RO_SLOT_PAD * (size_t)slot;
}

// One slot, one wave: the whole pass.  `slot` is the batch index, `req` the
// index relative to the offset tables passed in.
DEV void ro_slot(RoState& S, int req, int slot, const uint8_t* resp_bytes,
                 const uint32_t* resp_off, const int32_t* msg_idx_arr,
                 const uint8_t* id_slots, const SlotResult* enc_results,
                 uint8_t* scratch, const uint32_t* scratch_off,
                 uint8_t* final_out, const uint32_t* final_off,
                 DecodeResult* results, uint8_t* arena, int mode) {
  RoReq q;
  q.pb = resp_bytes + resp_off[req];
  q.wire_len = resp_off[req + 1] - resp_off[req];
  q.scr = scratch + scratch_off[req];
  q.scr_cap = scratch_off[req + 1] - scratch_off[req];
  q.fout = final_out + final_off[req];
  q.fcap = final_off[req + 1] - final_off[req];
  q.msg_idx = msg_idx_arr[req];
  q.idl = enc_results ? enc_results[req].id_len : 0;
  q.idp = id_slots + (size_t)req * ID_SLOT_BYTES;
  S.out = arena + ro_region(resp_off[req], slot);
  S.out_cap = 2 * q.wire_len + RO_SLOT_PAD;
  S.side = S.out + S.out_cap;
  S.side_cap = q.wire_len;
  if (!reorder_walk(S, q.pb, q.wire_len, q.msg_idx)) return;
  ro_redecode(S, q, mode, &results[req], final_off[req]);
}

#ifndef GGRMCP_HOST_SIM

// One wave per slot, grid-stride.  `work` holds RO_STACK_RUNS records per
// wave of the GRID (not per slot), so the launch caps the grid at
// RO_GRID_BLOCKS.  slot0 is the batch index of the tables' first slot.
extern "C" __global__ void __launch_bounds__(WPB * WAVE) k_pb_reorder(
    const uint8_t* __restrict__ resp_bytes,
    const uint32_t* __restrict__ resp_off,
    const int32_t* __restrict__ msg_idx_arr,
    const uint8_t* __restrict__ id_slots,
    const SlotResult* __restrict__ enc_results, uint8_t* __restrict__ scratch,
    const uint32_t* __restrict__ scratch_off, uint8_t* __restrict__ final_out,
    const uint32_t* __restrict__ final_off, DecodeResult* __restrict__ results,
    const int32_t* __restrict__ skip, uint8_t* __restrict__ arena,
    RoRec* __restrict__ work, Tables t, int n_req, int mode, int slot0) {
  __shared__ RoWin win[WPB];
  int wave_in_block = threadIdx.x / WAVE;
  RoState S;
  S.win = &win[wave_in_block];
  S.stack = work + (size_t)(blockIdx.x * WPB + wave_in_block) * RO_STACK_RUNS;
  S.lane = lane_id();
  S.t = t;
  for (int req = blockIdx.x * WPB + wave_in_block; req < n_req;
       req += gridDim.x * WPB) {
    if (skip && skip[req] == 1) continue;  // the host's slot
    if (results[req].status != E_UNSUPPORTED) continue;
    ro_slot(S, req, slot0 + req, resp_bytes, resp_off, msg_idx_arr, id_slots,
            enc_results, scratch, scratch_off, final_out, final_off, results,
            arena, mode);
  }
}

#else  // GGRMCP_HOST_SIM

// The kernel above on the CPU, one slot at a time.  `arena` is sized as
// ro_region describes; the window and the record stack are exact-size heap
// blocks so a sanitizer sees every bound.
inline void reorder_host(const uint8_t* resp_bytes, const uint32_t* resp_off,
                         const int32_t* msg_idx_arr, const uint8_t* id_slots,
                         const SlotResult* enc_results, uint8_t* scratch,
                         const uint32_t* scratch_off, uint8_t* final_out,
                         const uint32_t* final_off, DecodeResult* results,
                         const int32_t* skip, uint8_t* arena, const Tables& t,
                         int n_req, int mode) {
  RoWin* win = new RoWin;
  RoRec* work = new RoRec[RO_STACK_RUNS];
  RoState S;
  S.win = win;
  S.stack = work;
  S.lane = 0;
  S.t = t;
  threadIdx.x = 0;
  for (int req = 0; req < n_req; ++req) {
    if (skip && skip[req] == 1) continue;
    if (results[req].status != E_UNSUPPORTED) continue;
    ro_slot(S, req, req, resp_bytes, resp_off, msg_idx_arr, id_slots,
            enc_results, scratch, scratch_off, final_out, final_off, results,
            arena, mode);
  }
  delete[] work;
  delete win;
}

#endif  // GGRMCP_HOST_SIM
