// Packed numeric arrays on encode, one element per lane (gfx950; also the
// single-lane CPU build, where a window is one element).
//
// pk_window takes the JSON text of a packed `repeated` numeric field from an
// element start and commits as many leading elements as it can prove complete:
//
//   scan     256 bytes from `pos` become four position-ordered 64-bit masks
//            of ',' | ']' and four of ']' (wave-uniform ballots)
//   own      lane k owns the piece that ends at the k-th separator; it finds
//            that bit by rank-select over the masks (popcounts, no LDS) and its
//            start from lane k-1
//   parse    the lane trims whitespace and accepts its piece only as ONE
//            complete token: strict JSON number text, the same in quotes, or
//            for double/float the three quoted non-finite names.  The value
//            ends in a register (fpp_to_double below for double/float)
//   commit   one ballot of "valid"; the longest all-valid prefix is taken.  A
//            complete token cannot lie inside a string that began at an element
//            boundary, so the separators before and after it are real ones
//   place    fixed-width kinds at opos + width * k; varint kinds by an
//            inclusive __shfl_up scan of the lengths.  Only the elements that
//            fit below `ocap` are taken, judged before any lane stores
//   store    each lane stores its own bytes
//
// The window never reports an error: whatever it declines (odd spellings such
// as 1.0 in an integer field, leading zeros, escapes, out-of-range values,
// stray commas, an output that is full) is left at `pos` for the serial
// encode_packed_element, which then produces the status, err_pos and aux.
//
// fpp_to_double is an Eisel-Lemire style decimal-to-binary conversion in
// integer arithmetic only (D. Lemire, "Number parsing at a gigabyte per
// second", 2021): w * 10^q with w < 2^64 is w * 5^q * 2^q, 5^q comes from a
// 128-bit truncated table entry (pow5_table.h, generated and checked by
// tools/gen_pow10_table.py) and the 64x128 -> 192-bit product P bounds the
// true value V by P <= V < P + 2^64.  The 53-bit result is read off P when
// both ends of that bound round the same way, which fails only when every
// dropped bit above the low word is one.  Then V may be the boundary itself,
// which for -27 <= q < 0 is decided by whether 5^-q divides w; in every other
// such case the lane declines.  Correct over the whole range, subnormals and
// DBL_MAX included; no floating-point operation, so no fp pragma.
//
// docs/KERNELS.md rule 2 holds: no addressable per-lane temporaries; results
// travel as small structs in registers.  The entry points are DEVN and take
// scalars, not the walker's context, so the walkers' registers do not pay
// for them.
//
// Include after common.h (DEV, WAVE, is_ws, zigzag*, K_*) and the DEVN
// definition.
#pragma once

#include "fp_shortest.h"  // fps_mulhi, fps_flog2pow10
#include "pow5_table.h"

constexpr uint64_t FPP_DECLINED = ~0ull;  // a NaN pattern no conversion returns

// bits of the double nearest to w * 10^q (ties to even), or FPP_DECLINED where
// the product cannot decide, the result is not finite or a non-zero w
// underflows to zero.
DEVN uint64_t fpp_to_double(uint64_t w, int q) {
  if (w == 0) return 0;
  if (q < FPP_Q_MIN || q > FPP_Q_MAX) return FPP_DECLINED;
  const int lz = __builtin_clzll(w);
  const uint64_t wn = w << lz;
  const uint64_t th = FPP_T[2 * (q - FPP_Q_MIN)];
  const uint64_t tl = FPP_T[2 * (q - FPP_Q_MIN) + 1];
  // P = wn * (th * 2^64 + tl) = hi:mid:lo
  const uint64_t a_lo = wn * th, a_hi = fps_mulhi(wn, th);
  const uint64_t lo = wn * tl, b_hi = fps_mulhi(wn, tl);
  const uint64_t mid = a_lo + b_hi;
  const uint64_t hi = a_hi + (mid < a_lo ? 1 : 0);
  const int up = (int)(hi >> 63);  // P in [2^190, 2^192)
  // V = P * 2^x, x = floor(log2(5^q)) - 127 + q - lz
  const int fl2 = fps_flog2pow10(q) - q;
  int E = 190 + up + (fl2 - 127) + q - lz + 1023;  // biased exponent
  int t = 9 + up;  // bits of `hi` below the 53 + 1 kept ones
  if (E < 1) {     // subnormal: keep fewer
    t += 1 - E;
    E = 1;
  }
  if (t > 63) return FPP_DECLINED;  // below half the smallest subnormal
  uint64_t m = hi >> t;
  const uint64_t rmask = (1ull << t) - 1, rhi = hi & rmask;
  const bool exact = q >= 0 && q <= FPP_Q_EXACT;  // the entry is 5^q itself
  bool sticky;
  if (!exact && rhi == rmask && mid == ~0ull) {
    // P + 2^64 carries into the kept bits.  V is that boundary iff it is
    // w / 5^-q * 2^q with the division exact (then V has at most 64
    // significant bits, and the only multiple of 2^64 in range is the carry)
    if (q >= 0 || q < -27) return FPP_DECLINED;
    const uint64_t p5 =
        FPP_T[2 * (-q - FPP_Q_MIN)] >> (63 - (fps_flog2pow10(-q) + q));
    if (w % p5) return FPP_DECLINED;
    m += 1;
    sticky = false;
  } else {
    // a truncated entry puts V strictly above P
    sticky = !exact || (rhi | mid | lo) != 0;
  }
  uint64_t mant = m >> 1;
  if ((m & 1) && (sticky || (mant & 1))) ++mant;
  // mant carries the implicit bit (none when subnormal); a carry out of it
  // lands in the exponent field, which is the right answer
  const uint64_t bits = ((uint64_t)(E - 1) << 52) + mant;
  if (bits == 0 || bits >= 0x7ff0000000000000ull) return FPP_DECLINED;
  return bits;
}

struct PkVal {
  uint64_t v;  // payload: fixed-width bits or the varint's value
  bool ok;
};

// 8 bytes of s at p, zeros past n
DEV uint64_t pk_load8(const uint8_t* s, uint32_t p, uint32_t n) {
  uint64_t w = 0;
  if (p + 8 <= n) {
    __builtin_memcpy(&w, s + p, 8);  // unaligned ok on CDNA
    return w;
  }
  for (uint32_t j = 0; j < 8 && p + j < n; ++j) w |= (uint64_t)s[p + j] << (8 * j);
  return w;
}

DEV bool pk_lit(const uint8_t* s, uint32_t a, uint32_t b, const char* lit, uint32_t n) {
  if (b - a != n) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (s[a + i] != (uint8_t)lit[i]) return false;
  return true;
}

DEV bool pk_is_fp(uint32_t kind) { return kind == K_DOUBLE || kind == K_FLOAT; }
DEV uint32_t pk_fixed_width(uint32_t kind) {
  if (kind == K_DOUBLE || kind == K_FIXED64 || kind == K_SFIXED64) return 8;
  if (kind == K_FLOAT || kind == K_FIXED32 || kind == K_SFIXED32) return 4;
  return 0;
}

// one piece s[a, b), whitespace already trimmed, as an element of `kind`.
// Strict JSON number grammar -?(0|[1-9][0-9]*)(.[0-9]+)?([eE][+-]?[0-9]+)?
// (integer kinds: the first group only); everything else is not ok.
DEVN PkVal pk_parse_piece(const uint8_t* s, uint32_t n, uint32_t a, uint32_t b,
                          uint32_t kind) {
  PkVal r;
  r.v = 0;
  r.ok = false;
  const bool fp = pk_is_fp(kind);
  if (a < b && s[a] == '"') {
    if (b - a < 3 || s[b - 1] != '"') return r;
    ++a;
    --b;
    if (fp) {
      uint64_t nf = 0;
      if (pk_lit(s, a, b, "NaN", 3)) nf = 0x7ff8000000000000ull;
      else if (pk_lit(s, a, b, "Infinity", 8)) nf = 0x7ff0000000000000ull;
      else if (pk_lit(s, a, b, "-Infinity", 9)) nf = 0xfff0000000000000ull;
      if (nf) {
        r.v = kind == K_DOUBLE
                  ? nf
                  : (uint64_t)__builtin_bit_cast(
                        uint32_t, (float)__builtin_bit_cast(double, nf));
        r.ok = true;
        return r;
      }
    }
  }
  if (a >= b) return r;
  bool neg = false;
  if (s[a] == '-') {
    neg = true;
    if (++a >= b) return r;
  }
  enum { ST_START, ST_ZERO, ST_INT, ST_DOT, ST_FRAC, ST_E, ST_ESIGN, ST_EXP };
  int st = ST_START;
  uint64_t w = 0, cur = 0;
  int nd = 0;     // significant digits held in w (double/float: at most 19)
  int dexp = 0;   // decimal exponent that goes with w
  int ev = 0;     // explicit exponent
  bool eneg = false, dropped = false;
  for (uint32_t i = a; i < b; ++i) {
    if (((i - a) & 7) == 0) cur = pk_load8(s, i, n);
    const uint8_t ch = (uint8_t)cur;
    cur >>= 8;
    if (ch >= '0' && ch <= '9') {
      const uint32_t d = ch - '0';
      if (st >= ST_E) {
        st = ST_EXP;
        if (ev < 100000) ev = ev * 10 + (int)d;
        continue;
      }
      if (st == ST_ZERO) return r;  // leading zero
      const bool frac = st >= ST_DOT;
      st = frac ? ST_FRAC : (st == ST_START && d == 0 ? ST_ZERO : ST_INT);
      if (!fp) {
        // all 20 digits of a uint64, no more
        if (w > 1844674407370955161ull || (w == 1844674407370955161ull && d > 5))
          return r;
        w = w * 10 + d;
      } else if (nd < 19) {
        w = w * 10 + d;
        if (w) ++nd;
        if (frac) --dexp;
      } else {
        if (d) dropped = true;
        if (!frac) ++dexp;
      }
    } else if (ch == '.') {
      if (!fp || (st != ST_ZERO && st != ST_INT)) return r;
      st = ST_DOT;
    } else if (ch == 'e' || ch == 'E') {
      if (!fp || (st != ST_ZERO && st != ST_INT && st != ST_FRAC)) return r;
      st = ST_E;
    } else if (ch == '+' || ch == '-') {
      if (st != ST_E) return r;
      st = ST_ESIGN;
      eneg = ch == '-';
    } else {
      return r;  // quotes, backslashes, inner whitespace, letters
    }
  }
  if (st != ST_ZERO && st != ST_INT && st != ST_FRAC && st != ST_EXP) return r;

  if (fp) {
    const int q = dexp + (eneg ? -ev : ev);
    uint64_t bits = fpp_to_double(w, q);
    if (bits == FPP_DECLINED) return r;
    // digits were dropped: the text lies strictly between w and w + 1, and
    // rounding is monotone
    if (dropped && fpp_to_double(w + 1, q) != bits) return r;
    if (neg) bits |= 0x8000000000000000ull;
    if (kind == K_DOUBLE) {
      r.v = bits;
    } else {
      const float fv = (float)__builtin_bit_cast(double, bits);
      if (isinf(fv)) return r;  // finite text past FLT_MAX: the serial path rejects
      r.v = __builtin_bit_cast(uint32_t, fv);
    }
    r.ok = true;
    return r;
  }

  const bool is32 = kind == K_INT32 || kind == K_SINT32 || kind == K_SFIXED32 ||
                    kind == K_UINT32 || kind == K_FIXED32;
  const bool uns = kind == K_UINT64 || kind == K_FIXED64 || kind == K_UINT32 ||
                   kind == K_FIXED32;
  if (uns) {
    if ((neg && w) || (is32 && w > 0xffffffffull)) return r;
    r.v = w;
  } else {
    const uint64_t lim = is32 ? 0x80000000ull : 0x8000000000000000ull;
    if (w > lim - (neg ? 0 : 1)) return r;
    const int64_t v = (int64_t)(neg ? 0 - w : w);
    if (kind == K_SINT64) r.v = zigzag64(v);
    else if (kind == K_SINT32) r.v = zigzag32((int32_t)v);
    else if (kind == K_SFIXED32) r.v = (uint32_t)(int32_t)v;
    else r.v = (uint64_t)v;  // int32 sign-extends to ten bytes
  }
  r.ok = true;
  return r;
}

// ',' | ']' and ']' masks of s[base, base + 64), bit i = byte base + i
DEV void pk_scan64(const uint8_t* s, uint32_t n, uint32_t base, int lane,
                   uint64_t& sep, uint64_t& cls) {
  uint64_t ms = 0, mc = 0;
  for (uint32_t i = (uint32_t)lane; i < 64; i += WAVE) {
    const uint32_t p = base + i;
    const uint8_t ch = p < n ? s[p] : 0;
    if (ch == ',' || ch == ']') ms |= 1ull << i;
    if (ch == ']') mc |= 1ull << i;
  }
#if WAVE > 1
  ms = __ballot(ms != 0);
  mc = __ballot(mc != 0);
#endif
  sep = ms;
  cls = mc;
}

constexpr uint32_t PK_STRETCH = 256;

struct PkWin {
  uint32_t pos, opos;  // wave-uniform, advanced past what was committed
  int32_t state;       // 0 nothing committed, 1 array goes on, 2 ']' consumed
};

// `pos` is at an element start (whitespace allowed), outside any string.
DEVN PkWin pk_window(const uint8_t* s, uint32_t n, uint32_t pos, uint8_t* out,
                     uint32_t opos, uint32_t ocap, int lane, uint32_t kind) {
  PkWin res;
  res.pos = pos;
  res.opos = opos;
  res.state = 0;
  uint64_t s0, s1, s2, s3, r0, r1, r2, r3;
  pk_scan64(s, n, pos, lane, s0, r0);
  pk_scan64(s, n, pos + 64, lane, s1, r1);
  pk_scan64(s, n, pos + 128, lane, s2, r2);
  pk_scan64(s, n, pos + 192, lane, s3, r3);
  const uint32_t c0 = (uint32_t)__builtin_popcountll(s0);
  const uint32_t c1 = c0 + (uint32_t)__builtin_popcountll(s1);
  const uint32_t c2 = c1 + (uint32_t)__builtin_popcountll(s2);
  const uint32_t c3 = c2 + (uint32_t)__builtin_popcountll(s3);
  // elements in the window: up to the first ']', the last separator, WAVE
  uint32_t cnt = c3;
  bool closes = true;
  if (r0) cnt = (uint32_t)__builtin_popcountll(s0 & ((r0 & (0 - r0)) - 1)) + 1;
  else if (r1) cnt = c0 + (uint32_t)__builtin_popcountll(s1 & ((r1 & (0 - r1)) - 1)) + 1;
  else if (r2) cnt = c1 + (uint32_t)__builtin_popcountll(s2 & ((r2 & (0 - r2)) - 1)) + 1;
  else if (r3) cnt = c2 + (uint32_t)__builtin_popcountll(s3 & ((r3 & (0 - r3)) - 1)) + 1;
  else closes = false;
  if (cnt > WAVE) {
    cnt = WAVE;
    closes = false;
  }
  if (cnt == 0) return res;

  // lane k: the k-th separator ends its piece
  const uint32_t k = (uint32_t)lane;
  const bool act = k < cnt;
  uint32_t end = pos;
  if (act) {
    const uint32_t j = k < c0 ? 0 : k < c1 ? 1 : k < c2 ? 2 : 3;
    const uint64_t m = j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3;
    const uint32_t below = j == 0 ? 0 : j == 1 ? c0 : j == 2 ? c1 : c2;
    end = pos + 64 * j + pk_select64(m, k - below);
  }
  const uint32_t prev = __shfl_up(end, 1, WAVE);
  uint32_t a = lane ? prev + 1 : pos, b = end;
  PkVal pv;
  pv.v = 0;
  pv.ok = false;
  if (act) {
    while (a < b && is_ws(s[a])) ++a;
    while (b > a && is_ws(s[b - 1])) --b;
    pv = pk_parse_piece(s, n, a, b, kind);
  }

  // longest all-valid prefix
  const uint64_t bad = ~__ballot(act && pv.ok);
  uint32_t take = bad ? (uint32_t)__ffsll((long long)bad) - 1 : 64;
  if (take > cnt) take = cnt;
  if (take == 0) return res;

  // place
  const uint32_t width = pk_fixed_width(kind);
  uint32_t len = 0;
  if (k < take) {
    len = width;
    if (!width) {
      len = 1;
      for (uint64_t v = pv.v; v >= 0x80; v >>= 7) ++len;
    }
  }
  uint32_t inc = width * (k + 1);
  if (!width) {
    inc = len;
    #pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const uint32_t upv = __shfl_up(inc, d, WAVE);
      if (lane >= d) inc += upv;
    }
  }
  // only what fits is taken; an element that does not is the serial path's
  // E_OVERFLOW to report
  const uint64_t fits = __ballot(k < take && opos + inc <= ocap);
  take = (uint32_t)__builtin_popcountll(fits);
  if (take == 0) return res;

  // store
  if (k < take) {
    uint8_t* at = out + opos + (inc - len);
    uint64_t v = pv.v;
    if (width) {
      for (uint32_t i = 0; i < width; ++i) at[i] = (uint8_t)(v >> (8 * i));
    } else {
      for (uint32_t i = 0; i + 1 < len; ++i) {
        at[i] = (uint8_t)(v | 0x80);
        v >>= 7;
      }
      at[len - 1] = (uint8_t)v;
    }
  }
  res.opos = opos + (uint32_t)__shfl(inc, (int)take - 1, WAVE);
  res.pos = (uint32_t)__shfl(end, (int)take - 1, WAVE) + 1;
  res.state = (closes && take == cnt) ? 2 : 1;
  return res;
}
