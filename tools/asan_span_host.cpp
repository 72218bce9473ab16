// Stand-alone sanitizer run of the native spans' pure host pieces
// (csrc/span_host.h): the gRPC reply parser over every byte-prefix of a
// 300-byte frame (a prefix of 16 bytes or more is an exact-size heap string,
// so a read past the delivered bytes is a finding; shorter ones sit in the
// string object and are judged by the verdict alone) and over the cases of
// tests/test_span_host.py, and both error-envelope builders over all 256
// single-byte details and every id shape.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -DGGRMCP_HOST_SIM -DWAVE=1 -Iggrmcp_amd/ops/csrc \
//       tools/asan_span_host.cpp -o /tmp/asan_span_host && /tmp/asan_span_host

#include <cstdio>
#include <cstring>
#include <string>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "span_host.h"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace spanhost;

static unsigned failures = 0;

static void expect(const char* what, int status, const std::string& data,
                   const std::string& msg, int want_status, size_t want_off,
                   size_t want_len, const char* want_err) {
  GrpcReply g = parse_grpc_reply(status, data, msg);
  bool ok = g.status == want_status && g.off == want_off && g.len == want_len &&
            (want_err ? g.err && !strcmp(g.err, want_err) : g.err == nullptr);
  // a payload span must lie inside the delivered bytes
  if (g.status == 0 && g.off + g.len > data.size()) ok = false;
  if (!ok) {
    fprintf(stderr, "%s: got (%d, %zu, %zu, %s)\n", what, g.status, g.off,
            g.len, g.err ? g.err : "null");
    ++failures;
  }
}

static std::string frame(uint8_t flag, uint32_t declared, size_t payload) {
  std::string f;
  f.push_back((char)flag);
  for (int s = 24; s >= 0; s -= 8) f.push_back((char)(declared >> s));
  for (size_t i = 0; i < payload; ++i) f.push_back((char)('a' + i % 26));
  return f;
}

int main() {
  // every byte-prefix of a 300-byte frame, plain and compressed
  for (uint8_t flag = 0; flag < 2; ++flag) {
    const std::string whole = frame(flag, 295, 295);
    for (size_t n = 0; n <= whole.size(); ++n) {
      std::string data(whole.data(), n);
      data.shrink_to_fit();
      if (n == 0)
        expect("prefix 0", 0, data, "", 0, 0, 0, nullptr);
      else if (n < 5)
        expect("prefix <5", 0, data, "", 13, 0, 0, GRPC_TRUNCATED);
      else if (flag)
        expect("prefix compressed", 0, data, "", 13, 0, 0, GRPC_COMPRESSED);
      else if (n < whole.size())
        expect("prefix short", 0, data, "", 13, 0, 0, GRPC_TRUNCATED);
      else
        expect("whole", 0, data, "", 0, 5, 295, nullptr);
      expect("prefix statusless", -1, data, "", 2, 0, 0, GRPC_NO_STATUS);
      expect("prefix status 5", 5, data, "gone", 5, 0, 0, "gone");
    }
  }
  expect("empty frame", 0, frame(0, 0, 0), "", 0, 5, 0, nullptr);
  expect("trailing bytes", 0, frame(0, 3, 3) + "tail", "", 0, 5, 3, nullptr);
  expect("declared 4, has 3", 0, frame(0, 4, 3), "", 13, 0, 0, GRPC_TRUNCATED);
  expect("declared 2^32-1", 0, frame(0, 0xFFFFFFFFu, 0), "", 13, 0, 0,
         GRPC_TRUNCATED);
  expect("compressed", 0, frame(1, 0, 0), "", 13, 0, 0, GRPC_COMPRESSED);
  expect("compressed, short", 0, frame(1, 4, 3), "", 13, 0, 0, GRPC_COMPRESSED);
  expect("statusless + msg", -1, "", "peer reset", 2, 0, 0, "peer reset");

  // both envelope builders over all 256 single-byte details, every id shape
  const std::string ids[] = {"1", "\"a\\\"b\"", std::string(64, '7')};
  size_t bytes = 0;
  for (int c = 0; c < 256; ++c) {
    const char detail[2] = {(char)c, 0};
    for (int k = 0; k < 4; ++k) {
      const char* id = k < 3 ? ids[k].data() : nullptr;
      size_t id_len = k < 3 ? ids[k].size() : 0;
      std::string out = "stale";
      rpc_error_envelope(out, id, id_len, -32603, detail);
      bytes += out.size();
      if (out.rfind("{\"jsonrpc\":\"2.0\",\"id\":", 0) != 0) ++failures;
      grpc_error_envelope(out, id, id_len, c % 19 - 1, detail);
      bytes += out.size();
      // control bytes never reach the envelope raw
      for (char ch : out)
        if ((unsigned char)ch < 0x20) ++failures;
    }
  }
  for (int s = -1; s < 10; ++s) {
    int code;
    const char* msg;
    status_to_rpc(s, &code, &msg);
    bytes += strlen(msg);
  }
  if (failures) return fprintf(stderr, "%u failures\n", failures), 1;
  printf("reply parser and envelopes ok (%zu envelope bytes), no sanitizer "
         "report\n", bytes);
  return 0;
}
