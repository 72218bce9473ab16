// ---------------------------------------------------------------------------
// k_pb2json_wg — workgroup-per-request decode for LARGE responses
// (BASELINE config 3: 64 KB payloads).  Included at the end of pb2json.hip.
//
// The per-wave walker serializes one request through 64 lanes at a
// ~26 us/KB floor (a 64 KB response costs ~1.7 ms of wave latency and the
// whole batch inherits it).  Here one WORKGROUP (WG_DEC_WAVES wave64s)
// owns one request:
//   A. one thread scans the top-level wire for contiguous field runs
//      ("items") — O(#fields), just varint/tag walking;
//   B. waves grab items dynamically and decode each item with the SAME
//      decode_walk machinery (bare_top: no surrounding braces) into a
//      private scratch region;
//   C. one thread cuts the item texts into slices, every wave measures the
//      escaped length of its slices, one thread prefix-sums them into final
//      offsets (comma-joined, skipping default-omitted empty items);
//   D. wave 0 writes the JSON-RPC envelope framing while every wave
//      escape-copies its slices into place.
// Requests the scanner cannot split safely (WKT-typed top message,
// out-of-order top fields, > WG_DEC_MAX_ITEMS runs) take the classic
// single-wave pass inside the same block, preserving exact semantics.
//
// Both decode flags are honoured, with k_pb2json's bytes:
//   DM_UNPOPULATED  a bare-top item walk fills no top-level gap (decode_walk);
//                   the scanner makes every top-level gap that holds a
//                   no-presence field a FILL ITEM in document order, and
//                   wave 0 prints them all into an area of their own
//                   (wgd_fill).  An unknown field, a known field in a
//                   foreign wire type and an empty packed run do not advance
//                   the classic walker's prev_number; a request that carries
//                   one at the top level takes the classic pass.
//   DM_STRUCTURED   the offset pass also lays out the raw second copy, and
//                   the copy pass writes every slice twice.
//
// Every phase is a DEV function over one WgDecState — __shared__ in the
// kernel, an ordinary object in the CPU build, where wg_decode_host calls the
// same phases one wave index at a time (WAVE=1) so the scanner, the joiner
// and the offset arithmetic run under the CPU tier's tests and sanitizers.
// The engine routes kind-0 slots with wire_len >= WG_DEC_MIN_BYTES here
// (skip tag == 2).  DecodeResult.pad tells which pass answered: 1 = items,
// 2 = the in-block classic pass (k_pb2json writes 0).
// ---------------------------------------------------------------------------
#pragma once

static __device__ const char WG_P1[] = "{\"jsonrpc\":\"2.0\",\"id\":";
static __device__ const char WG_P2[] =
    ",\"result\":{\"content\":[{\"type\":\"text\",\"text\":\"";
static __device__ const char WG_P3[] = "\"}],\"isError\":false}}";
static __device__ const char WG_S1[] = "\"}],\"structuredContent\":";
static __device__ const char WG_S2[] = ",\"isError\":false}}";

// items = top-level field runs; slices = fixed-size spans of the items'
// produced text, so the escape passes load-balance across waves even
// when one map/array run carries most of the payload
constexpr int WG_DEC_MAX_SLICES = 1024;

struct WgDecState {
  uint32_t start[WG_DEC_MAX_ITEMS + 1];  // item wire ranges
  // trimmed text of each item: length, and offset in the slot's scratch.
  // A fill item (empty wire range) parks its gap (lo, hi) in the pair until
  // wgd_fill replaces it with the printed text's (length, offset).
  uint32_t outlen[WG_DEC_MAX_ITEMS];
  uint32_t src[WG_DEC_MAX_ITEMS];
  // map / repeated runs are CHUNKED at entry boundaries so one big run
  // doesn't serialize on a single wave; each chunk's walk emits the full
  // `"name":{...}` / `"name":[...]` syntax and the joiner trims
  // head bytes of leading name syntax and tail closing brackets
  uint16_t head[WG_DEC_MAX_ITEMS];
  uint8_t tail[WG_DEC_MAX_ITEMS];
  uint16_t sl_item[WG_DEC_MAX_SLICES];
  uint32_t sl_off[WG_DEC_MAX_SLICES];   // offset within the item text
  uint32_t sl_esc[WG_DEC_MAX_SLICES];   // escaped length of the slice
  uint32_t sl_fin[WG_DEC_MAX_SLICES];   // final-buffer offset, escaped copy
  uint32_t sl_raw[WG_DEC_MAX_SLICES];   // final-buffer offset, raw copy
  uint8_t sl_comma[WG_DEC_MAX_SLICES];  // prepend ',' (item starts)
  int nitems, nslices, next, err, mode;
  uint32_t total, slice_bytes, text_end;
};

// one routed slot
struct WgDecReq {
  const uint8_t* pb;
  uint32_t wire_len;
  uint8_t* scr;
  uint32_t scr_cap;
  uint8_t* fout;
  uint32_t fcap;
  int msg_idx;
  const uint8_t* idp;  // request id token (idl bytes; "null" when 0)
  uint32_t idl;
  int flags;           // the mode's DM_UNPOPULATED / DM_STRUCTURED bits
  int max_phase;       // debug bisection knob (GGRMCP_WG_PHASES; 3 = all)
};

DEV bool wgd_is_fill(const WgDecState& S, int i) {
  return S.start[i] == S.start[i + 1];
}

// the fill area: past every item region the slot can hold
DEV uint32_t wgd_fill_base(const WgDecReq& q) {
  return 8u * q.wire_len + WG_DEC_ITEM_PAD * (uint32_t)WG_DEC_MAX_ITEMS;
}

// does message m have a field in the open interval (lo, hi) that
// fill_unpopulated would print?
DEV bool wgd_gap(const Tables& t, const MsgEntry& m, uint32_t lo, uint32_t hi) {
  for (int fi = 0; fi < m.field_count; ++fi) {
    const FieldEntry& fe = t.fields[m.field_start + fi];
    if (fe.number <= lo) continue;
    if (fe.number >= hi) break;  // sorted by number (tables.py)
    if (!(fe.flags & (F_HAS_PRESENCE | F_ONEOF))) return true;
  }
  return false;
}

DEV void wgd_ctx(DCtx& c, const Tables& t, uint8_t* out, uint32_t cap) {
  c.pb = nullptr;
  c.len = 0;
  c.pos = 0;
  c.out = out;
  c.opos = 0;
  c.ocap = cap;
  c.t = t;
  c.status = E_OK;
  c.lane = lane_id();
}

// ---- phase A: top-level field-run scan (one thread) -----------------------
// Runs group contiguous same-number tags; MAP / REPEATED runs split into
// ~4 KB chunks at entry boundaries (chunk walks re-emit the name syntax;
// head/tail trim it at join time) so a payload-dominating map field
// parallelizes across waves instead of serializing on one.
DEV void wgd_scan(WgDecState& S, const WgDecReq& q, const Tables& t) {
  if (threadIdx.x != 0) return;
  const uint8_t* pb = q.pb;
  const uint32_t wire_len = q.wire_len;
  const bool unpop = (q.flags & DM_UNPOPULATED) != 0;
  S.next = 0;
  S.err = E_OK;
  S.mode = 1;
  int n = 0;
  uint32_t pos = 0, prev_num = 0, cur = 0xFFFFFFFFu;
  uint32_t chunk_head = 0;   // head trim for continuation chunks of cur
  bool cur_split = false;    // cur run may chunk at entry boundaries
  uint32_t chunk_wire = 0;   // wire bytes accumulated in the open chunk
  const FieldEntry* cur_fe = nullptr;
  const MsgEntry& tm = t.msgs[q.msg_idx];
  bool ok = tm.wkt_kind == WKT_NONE;
  while (ok && pos < wire_len) {
    uint32_t tag_start = pos;
    uint64_t tag;
    if (!get_varint(pb, wire_len, &pos, &tag)) { ok = false; break; }
    uint32_t num = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (num == 0) { ok = false; break; }
    if (num != cur) {
      // close the previous run: its last chunk keeps the bracket
      if (n > 0) S.tail[n - 1] = 0;
      // new run must be strictly ascending (non-adjacent duplicates are
      // the classic path's E_UNSUPPORTED -> host fallback)
      if (num < prev_num || n >= WG_DEC_MAX_ITEMS) { ok = false; break; }
      // field lookup decides chunkability (maps + per-entry repeated)
      cur_split = false;
      chunk_head = 0;
      cur_fe = nullptr;
      for (int fi = 0; fi < tm.field_count; ++fi) {
        const FieldEntry& fe = t.fields[tm.field_start + fi];
        if (fe.number != num) continue;
        cur_fe = &fe;
        bool per_entry_len =
            (fe.flags & F_MAP) ||
            ((fe.flags & F_REPEATED) &&
             (fe.kind == K_MESSAGE || fe.kind == K_STRING ||
              fe.kind == K_BYTES));
        // unpacked repeated scalars (wt != W_LEN run) also chunk
        bool per_entry_scalar =
            (fe.flags & F_REPEATED) && !(fe.flags & F_MAP) && wt != W_LEN;
        if (per_entry_len || per_entry_scalar) {
          cur_split = true;
          // `"name":{` / `"name":[` = 1 + json_len + 2 + 1 bytes
          chunk_head = (uint32_t)fe.json_len + 4;
        }
        break;
      }
      if (unpop) {
        // an unknown field leaves the classic walker's prev_number alone:
        // the gap after it starts further back than this scan knows
        if (cur_fe == nullptr) { ok = false; break; }
        if (wgd_gap(t, tm, prev_num, num)) {
          // the fill item and the run's first item must both fit
          if (n + 1 >= WG_DEC_MAX_ITEMS) { ok = false; break; }
          S.head[n] = 0;
          S.tail[n] = 0;
          S.outlen[n] = prev_num;
          S.src[n] = num;
          S.start[n++] = tag_start;
        }
      }
      S.head[n] = 0;
      S.tail[n] = (uint8_t)(cur_split ? 1 : 0);
      S.start[n++] = tag_start;
      prev_num = num;
      cur = num;
      chunk_wire = 0;
    } else if (cur_split && chunk_wire >= 4096) {
      // continuation chunk of the same run at an entry boundary
      if (n >= WG_DEC_MAX_ITEMS) { ok = false; break; }
      S.head[n] = (uint16_t)chunk_head;
      S.tail[n] = 1;
      S.start[n++] = tag_start;
      chunk_wire = 0;
    }
    // under DM_UNPOPULATED a foreign wire type is an unknown field too
    bool packed_run = false;
    if (unpop) {
      uint32_t ew = expected_wire(*cur_fe);
      bool rep = (cur_fe->flags & F_REPEATED) != 0;
      if (wt != ew && !(rep && wt == W_LEN)) { ok = false; break; }
      packed_run = rep && wt == W_LEN && ew != W_LEN;
    }
    if (wt == W_VARINT) {
      uint64_t v;
      if (!get_varint(pb, wire_len, &pos, &v)) { ok = false; break; }
    } else if (wt == W_I64) {
      if (pos + 8 > wire_len) { ok = false; break; }
      pos += 8;
    } else if (wt == W_I32) {
      if (pos + 4 > wire_len) { ok = false; break; }
      pos += 4;
    } else if (wt == W_LEN) {
      uint64_t v;
      if (!get_varint(pb, wire_len, &pos, &v)) { ok = false; break; }
      if (v > wire_len - pos) { ok = false; break; }
      // ... and an empty packed run is no occurrence of its field
      if (packed_run && v == 0) { ok = false; break; }
      pos += (uint32_t)v;
    } else {
      ok = false;
      break;
    }
    chunk_wire += pos - tag_start;
  }
  if (ok && pos == wire_len && n > 0) {
    S.tail[n - 1] = 0;  // the wire's last chunk keeps its bracket
    if (unpop && wgd_gap(t, tm, prev_num, 0xFFFFFFFFu)) {
      if (n >= WG_DEC_MAX_ITEMS) {
        ok = false;
      } else {
        S.head[n] = 0;
        S.tail[n] = 0;
        S.outlen[n] = prev_num;
        S.src[n] = 0xFFFFFFFFu;
        S.start[n++] = wire_len;
      }
    }
  } else {
    ok = false;
  }
  if (ok) {
    S.start[n] = wire_len;
    S.nitems = n;
  } else {
    S.mode = 0;  // classic single-wave pass (wgd_classic)
    S.nitems = 0;
  }
}

// ---- phase B, fills: wave 0 prints every top-level gap, consecutively, into
// the fill area (bounded by the top message's field count); a two-byte item
// could never hold the defaults of the 58 fields before it ----------------
DEV void wgd_fill(WgDecState& S, const WgDecReq& q, const Tables& t) {
  if (!(q.flags & DM_UNPOPULATED) || threadIdx.x / WAVE != 0) return;
  const int lane = lane_id();
  const int n_items = S.nitems;
  const uint32_t base = wgd_fill_base(q);
  const uint32_t cap = q.scr_cap > base ? q.scr_cap - base : 0;
  DCtx c;
  wgd_ctx(c, t, cap ? q.scr + base : q.scr, cap);
  c.unpop = DM_UNPOPULATED;
  bool dead = false;
  for (int i = 0; i < n_items; ++i) {
    if (!wgd_is_fill(S, i)) continue;
    uint32_t lo = S.outlen[i], hi = S.src[i], at = c.opos;
    uint8_t first = 1;
    if (!dead && !fill_unpopulated(c, q.msg_idx, lo, hi, &first)) {
      dead = true;
      if (!lane) atomicCAS(&S.err, E_OK, c.status == E_OK ? E_PARSE : c.status);
    }
    if (!lane) {
      S.src[i] = base + at;
      S.outlen[i] = dead ? 0 : c.opos - at;
    }
  }
}

// ---- phase B, items: decode (dynamic wave grabs; the guard bound makes
// the loop provably finite — a wave can win at most n_items grabs) ----------
DEV void wgd_walk(WgDecState& S, const WgDecReq& q, const Tables& t) {
  const int lane = lane_id();
  const int n_items = S.nitems;
  for (int guard = 0; guard <= WG_DEC_MAX_ITEMS + 1; ++guard) {
    int idx = 0;
    if (!lane) idx = atomicAdd(&S.next, 1);
    idx = __shfl(idx, 0, WAVE);
    if (idx >= n_items) break;
    if (wgd_is_fill(S, idx)) continue;  // wgd_fill's
    uint32_t ist = S.start[idx], ien = S.start[idx + 1];
    uint32_t soff = 8u * ist + WG_DEC_ITEM_PAD * (uint32_t)idx;
    uint32_t scap = 8u * (ien - ist) + WG_DEC_ITEM_PAD;
    if (soff + scap > q.scr_cap) {
      if (!lane) {
        atomicCAS(&S.err, E_OK, E_OVERFLOW);
        S.outlen[idx] = 0;
        S.src[idx] = 0;
      }
      continue;
    }
    DCtx c;
    wgd_ctx(c, t, q.scr + soff, scap);
    c.pb = q.pb;
    c.len = ien;
    c.pos = ist;
    c.unpop = (uint32_t)(q.flags & DM_UNPOPULATED);
    bool ok = decode_walk(c, q.msg_idx, ien, /*bare_top=*/true);
    uint32_t trim = (uint32_t)S.head[idx] + S.tail[idx];
    if (!ok || c.status != E_OK || c.opos < trim) {
      if (!lane) {
        atomicCAS(&S.err, E_OK, c.status == E_OK ? E_PARSE : c.status);
        S.outlen[idx] = 0;
        S.src[idx] = 0;
      }
      continue;
    }
    // store the TRIMMED text (chunk joins drop re-emitted name syntax
    // and the premature closing bracket)
    if (!lane) {
      S.outlen[idx] = c.opos - trim;
      S.src[idx] = soff + S.head[idx];
    }
  }
}

// ---- phase C1: slice the item texts (one thread) --------------------------
DEV void wgd_slice(WgDecState& S) {
  if (!S.mode || threadIdx.x != 0) return;
  const int n_items = S.nitems;
  S.next = 0;
  int ns = 0;
  if (S.err == E_OK) {
    uint32_t sum = 0;
    for (int i = 0; i < n_items; ++i) sum += S.outlen[i];
    uint32_t sb = 4096;
    uint32_t budget = (uint32_t)(WG_DEC_MAX_SLICES - n_items);
    if (budget > 0 && sum / budget + 1 > sb) sb = sum / budget + 1;
    S.slice_bytes = sb;
    bool clipped = false;
    for (int i = 0; i < n_items && !clipped; ++i) {
      for (uint32_t off = 0; off < S.outlen[i]; off += sb) {
        if (ns >= WG_DEC_MAX_SLICES) {  // unreachable by the budget math
          clipped = true;               // above, but NEVER truncate output
          break;                        // silently
        }
        S.sl_item[ns] = (uint16_t)i;
        S.sl_off[ns] = off;
        ++ns;
      }
    }
    if (clipped) S.err = E_OVERFLOW;
  }
  S.nslices = ns;
}

DEV uint32_t wgd_slice_len(const WgDecState& S, int s) {
  uint32_t ilen = S.outlen[S.sl_item[s]] - S.sl_off[s];
  return ilen > S.slice_bytes ? S.slice_bytes : ilen;
}

// ---- phase C2: escaped length per slice (wave-parallel) -------------------
// static wave-strided assignment: slices are uniform-size, so dynamic
// grabbing buys nothing over round-robin
DEV void wgd_esclen(WgDecState& S, const WgDecReq& q) {
  if (!S.mode || S.err != E_OK || q.max_phase < 2) return;
  const int lane = lane_id();
  const int wave = threadIdx.x / WAVE;
  const int n_slices = S.nslices;
  for (int s = wave; s < n_slices; s += WG_DEC_WAVES) {
    uint32_t ilen = wgd_slice_len(S, s);
    const uint8_t* src = q.scr + S.src[S.sl_item[s]] + S.sl_off[s];
    uint32_t acc = 0;
    for (uint32_t i = lane; i < ilen; i += WAVE) acc += esc_len(src[i]);
    for (int d = WAVE / 2; d > 0; d >>= 1) acc += __shfl_down(acc, d, WAVE);
    if (!lane) S.sl_esc[s] = acc;
  }
}

// ---- phase C3: prefix sums + envelope sizing (one thread) -----------------
// Nothing is written before `total > fcap` has been judged.
DEV void wgd_offsets(WgDecState& S, const WgDecReq& q) {
  if (!S.mode || threadIdx.x != 0) return;
  S.next = 0;
  if (S.err != E_OK) return;
  const int n_slices = S.nslices;
  uint32_t pre = (uint32_t)(sizeof(WG_P1) - 1) + (q.idl ? q.idl : 4) +
                 (uint32_t)(sizeof(WG_P2) - 1) + 1 /* '{' */;
  uint32_t off = pre, raw = 0;
  int first = 1;
  for (int s = 0; s < n_slices; ++s) {
    uint8_t comma = 0;
    if (S.sl_off[s] == 0) {  // first slice of its item
      if (!first) comma = 1;
      first = 0;
    }
    S.sl_comma[s] = comma;
    off += comma;
    S.sl_fin[s] = off;
    off += S.sl_esc[s];
    raw += comma;
    S.sl_raw[s] = raw;  // relative until the text block's end is known
    raw += wgd_slice_len(S, s);
  }
  S.text_end = off;  // where the text object's '}' goes
  uint32_t total;
  if (q.flags & DM_STRUCTURED) {
    // '}' S1 '{' raw join '}' S2
    uint32_t rbase = off + 1 + (uint32_t)(sizeof(WG_S1) - 1) + 1;
    for (int s = 0; s < n_slices; ++s) S.sl_raw[s] += rbase;
    total = rbase + raw + 1 + (uint32_t)(sizeof(WG_S2) - 1);
  } else {
    total = off + 1 /* '}' */ + (uint32_t)(sizeof(WG_P3) - 1);
  }
  if (total > q.fcap) S.err = E_OVERFLOW;
  S.total = total;
}

// ---- phase D: envelope framing (wave 0) + slice copies (all waves) --------
DEV void wgd_copy(WgDecState& S, const WgDecReq& q, const Tables& t) {
  if (!S.mode || S.err != E_OK || q.max_phase < 3) return;
  const int lane = lane_id();
  const int wave = threadIdx.x / WAVE;
  const int n_slices = S.nslices;
  const bool structured = (q.flags & DM_STRUCTURED) != 0;
  uint8_t* fout = q.fout;
  if (wave == 0) {
    DCtx o;
    wgd_ctx(o, t, fout, q.fcap);
    bool ok = puts_(o, WG_P1, sizeof(WG_P1) - 1);
    if (ok && q.idl) {
      for (uint32_t i = lane; i < q.idl; i += WAVE) o.out[o.opos + i] = q.idp[i];
      o.opos += q.idl;
    } else if (ok) {
      ok = puts_(o, "null", 4);
    }
    if (ok) ok = puts_(o, WG_P2, sizeof(WG_P2) - 1);
    if (ok) ok = putc_(o, '{');
    // the text object's '}' and what follows it, at the precomputed spots
    uint32_t cpos = S.text_end;
    if (!lane) fout[cpos] = '}';
    if (structured) {
      for (uint32_t i = lane; i < sizeof(WG_S1) - 1; i += WAVE)
        fout[cpos + 1 + i] = (uint8_t)WG_S1[i];
      uint32_t epos = S.total - (uint32_t)(sizeof(WG_S2) - 1) - 1;
      if (!lane) {
        fout[cpos + (uint32_t)sizeof(WG_S1)] = '{';
        fout[epos] = '}';
      }
      for (uint32_t i = lane; i < sizeof(WG_S2) - 1; i += WAVE)
        fout[epos + 1 + i] = (uint8_t)WG_S2[i];
    } else {
      for (uint32_t i = lane; i < sizeof(WG_P3) - 1; i += WAVE)
        fout[cpos + 1 + i] = (uint8_t)WG_P3[i];
    }
    if (!ok && !lane) atomicCAS(&S.err, E_OK, o.status);
  }
  for (int s = wave; s < n_slices; s += WG_DEC_WAVES) {
    uint32_t ilen = wgd_slice_len(S, s);
    const uint8_t* src = q.scr + S.src[S.sl_item[s]] + S.sl_off[s];
    if (S.sl_comma[s] && !lane) fout[S.sl_fin[s] - 1] = ',';
    DCtx e;
    wgd_ctx(e, t, fout + S.sl_fin[s], S.sl_esc[s]);
    // slice of already-validated walker output: skip the UTF-8 re-check
    // (a boundary can split a multi-byte char; escaping is per-byte)
    if (!put_escaped(e, src, ilen, /*validate=*/false)) {
      if (!lane) atomicCAS(&S.err, E_OK, e.status);
    }
    if (structured) {
      // the same slice once more, raw, with the same comma
      uint8_t* dst = fout + S.sl_raw[s];
      if (S.sl_comma[s] && !lane) dst[-1] = ',';
      for (uint32_t i = lane; i < ilen; i += WAVE) dst[i] = src[i];
    }
  }
}

// ---- the classic single-wave pass (k_pb2json's kind-0 body, same bytes) ---
DEV void wgd_classic(WgDecState& S, const WgDecReq& q, const Tables& t,
                     DecodeResult* result, uint32_t out_off) {
  if (S.mode || threadIdx.x / WAVE != 0) return;
  const int lane = lane_id();
  DecodeResult r;
  r.status = E_OK;
  r.out_off = out_off;
  r.out_len = 0;
  r.pad = 2;
  DCtx c;
  wgd_ctx(c, t, q.scr, q.scr_cap);
  c.pb = q.pb;
  c.len = q.wire_len;
  c.unpop = (uint32_t)(q.flags & DM_UNPOPULATED);
  decode_walk(c, q.msg_idx, c.len);
  if (c.status != E_OK) {
    r.status = c.status;
    if (!lane) *result = r;
    return;
  }
  uint32_t json_len = c.opos;
  DCtx o;
  wgd_ctx(o, t, q.fout, q.fcap);
  bool ok = puts_(o, WG_P1, sizeof(WG_P1) - 1);
  if (ok && q.idl) {
    if (o.opos + q.idl > o.ocap) ok = dfail(o, E_OVERFLOW);
    if (ok) {
      for (uint32_t i = lane; i < q.idl; i += WAVE) o.out[o.opos + i] = q.idp[i];
      o.opos += q.idl;
    }
  } else if (ok) {
    ok = puts_(o, "null", 4);
  }
  if (ok) ok = puts_(o, WG_P2, sizeof(WG_P2) - 1);
  if (ok) ok = put_escaped(o, q.scr, json_len);
  if (ok && (q.flags & DM_STRUCTURED)) {
    ok = puts_(o, WG_S1, sizeof(WG_S1) - 1);
    if (ok && o.opos + json_len > o.ocap) ok = dfail(o, E_OVERFLOW);
    if (ok) {
      for (uint32_t i = lane; i < json_len; i += WAVE)
        o.out[o.opos + i] = q.scr[i];
      o.opos += json_len;
      ok = puts_(o, WG_S2, sizeof(WG_S2) - 1);
    }
  } else if (ok) {
    ok = puts_(o, WG_P3, sizeof(WG_P3) - 1);
  }
  if (!ok) {
    r.status = o.status;
  } else {
    r.out_len = o.opos;
  }
  if (!lane) *result = r;
}

// ---- finalize (item mode) -------------------------------------------------
DEV void wgd_finish(WgDecState& S, DecodeResult* result, uint32_t out_off) {
  if (!S.mode || threadIdx.x != 0) return;
  DecodeResult r;
  r.out_off = out_off;
  r.pad = 1;
  r.status = S.err;
  r.out_len = S.err == E_OK ? S.total : 0;
  *result = r;
}

DEV void wgd_req(WgDecReq& q, int req, const uint8_t* resp_bytes,
                 const uint32_t* resp_off, const int32_t* msg_idx_arr,
                 const uint8_t* id_slots, const SlotResult* enc_results,
                 uint8_t* scratch, const uint32_t* scratch_off,
                 uint8_t* final_out, const uint32_t* final_off, int mode,
                 int max_phase) {
  q.pb = resp_bytes + resp_off[req];
  q.wire_len = resp_off[req + 1] - resp_off[req];
  q.scr = scratch + scratch_off[req];
  q.scr_cap = scratch_off[req + 1] - scratch_off[req];
  q.fout = final_out + final_off[req];
  q.fcap = final_off[req + 1] - final_off[req];
  q.msg_idx = msg_idx_arr[req];
  q.idl = enc_results ? enc_results[req].id_len : 0;
  q.idp = id_slots + (size_t)req * ID_SLOT_BYTES;
  q.flags = mode & (DM_UNPOPULATED | DM_STRUCTURED);
  q.max_phase = max_phase;
}

#ifndef GGRMCP_HOST_SIM

// Every barrier is reached by all waves; what decides control flow between
// two barriers (S.mode, S.err, the counts) was written before the earlier one.
extern "C" __global__ void __launch_bounds__(WG_DEC_WAVES * WAVE) k_pb2json_wg(
    const uint8_t* __restrict__ resp_bytes,
    const uint32_t* __restrict__ resp_off,
    const int32_t* __restrict__ msg_idx_arr,
    const uint8_t* __restrict__ id_slots,
    const SlotResult* __restrict__ enc_results, uint8_t* __restrict__ scratch,
    const uint32_t* __restrict__ scratch_off, uint8_t* __restrict__ final_out,
    const uint32_t* __restrict__ final_off, DecodeResult* __restrict__ results,
    const int32_t* __restrict__ skip, Tables t, int n_req, int mode,
    int max_phase) {
  int req = blockIdx.x;
  if (req >= n_req) return;
  if (!skip || skip[req] != 2) return;  // 2 = routed to this kernel
  __shared__ WgDecState S;
  WgDecReq q;
  wgd_req(q, req, resp_bytes, resp_off, msg_idx_arr, id_slots, enc_results,
          scratch, scratch_off, final_out, final_off, mode, max_phase);
  wgd_scan(S, q, t);
  __syncthreads();
  if (S.mode && max_phase >= 1) {
    wgd_fill(S, q, t);
    wgd_walk(S, q, t);
  }
  __syncthreads();
  wgd_slice(S);
  __syncthreads();
  wgd_esclen(S, q);
  __syncthreads();
  wgd_offsets(S, q);
  __syncthreads();
  wgd_copy(S, q, t);
  wgd_classic(S, q, t, &results[req], final_off[req]);
  __syncthreads();
  wgd_finish(S, &results[req], final_off[req]);
}

#else  // GGRMCP_HOST_SIM

// The kernel above on the CPU: the same phases over an ordinary state
// object, each one run for every wave index in turn (WAVE=1: a wave is one
// thread) where the kernel has a barrier.  Wave 0 wins every item grab.
inline void wg_decode_host(
    const uint8_t* resp_bytes, const uint32_t* resp_off,
    const int32_t* msg_idx_arr, const uint8_t* id_slots,
    const SlotResult* enc_results, uint8_t* scratch,
    const uint32_t* scratch_off, uint8_t* final_out, const uint32_t* final_off,
    DecodeResult* results, const int32_t* skip, const Tables& t, int n_req,
    int mode, int max_phase = 3) {
  WgDecState* S = new WgDecState;
  for (int req = 0; req < n_req; ++req) {
    if (!skip || skip[req] != 2) continue;
    WgDecReq q;
    wgd_req(q, req, resp_bytes, resp_off, msg_idx_arr, id_slots, enc_results,
            scratch, scratch_off, final_out, final_off, mode, max_phase);
    auto waves = [&](auto phase) {
      for (int w = 0; w < WG_DEC_WAVES; ++w) {
        threadIdx.x = (unsigned)(w * WAVE);
        phase();
      }
      threadIdx.x = 0;
    };
    waves([&] { wgd_scan(*S, q, t); });
    if (S->mode && max_phase >= 1) {
      waves([&] { wgd_fill(*S, q, t); wgd_walk(*S, q, t); });
    }
    waves([&] { wgd_slice(*S); });
    waves([&] { wgd_esclen(*S, q); });
    waves([&] { wgd_offsets(*S, q); });
    waves([&] {
      wgd_copy(*S, q, t);
      wgd_classic(*S, q, t, &results[req], final_off[req]);
    });
    waves([&] { wgd_finish(*S, &results[req], final_off[req]); });
  }
  delete S;
}

#endif  // GGRMCP_HOST_SIM
