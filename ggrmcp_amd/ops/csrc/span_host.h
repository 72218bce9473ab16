// span_host.h — the pure host pieces of the native serving spans
// (Engine::process_span and Engine::run_span in engine.cpp): gRPC reply
// framing and the C++-assembled JSON-RPC error envelopes.  Nothing here
// touches HIP, pybind or the engine's state (common.h supplies the kernel
// status codes only), so _hostsim binds these functions for the CPU test
// tier (tests/test_span_host.py) and tools/asan_span_host.cpp runs them
// under the sanitizers.
#pragma once

#include <arpa/inet.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "common.h"

namespace spanhost {

// JSON string escaping for C++-assembled error envelopes (error details may
// contain quotes/control bytes)
inline void json_escape_append(std::string& out, const char* s, size_t n) {
  static const char* hex = "0123456789abcdef";
  for (size_t i = 0; i < n; ++i) {
    unsigned char c = (unsigned char)s[i];
    if (c == '"' || c == '\\') {
      out.push_back('\\');
      out.push_back((char)c);
    } else if (c == '\n') {
      out += "\\n";
    } else if (c == '\r') {
      out += "\\r";
    } else if (c == '\t') {
      out += "\\t";
    } else if (c < 0x20) {
      out += "\\u00";
      out.push_back(hex[c >> 4]);
      out.push_back(hex[c & 15]);
    } else {
      out.push_back((char)c);
    }
  }
}

// grpc status code -> canonical name (mirrors backend/native_invoker.py
// _CODE_NAMES so native and Python error texts match)
inline const char* grpc_status_name(int s) {
  static const char* names[] = {
      "OK", "CANCELLED", "UNKNOWN", "INVALID_ARGUMENT", "DEADLINE_EXCEEDED",
      "NOT_FOUND", "ALREADY_EXISTS", "PERMISSION_DENIED", "RESOURCE_EXHAUSTED",
      "FAILED_PRECONDITION", "ABORTED", "OUT_OF_RANGE", "UNIMPLEMENTED",
      "INTERNAL", "UNAVAILABLE", "DATA_LOSS", "UNAUTHENTICATED"};
  return (s >= 0 && s < 17) ? names[s] : "CODE_?";
}

// kernel status -> JSON-RPC (code, message); mirrors engine/batch.py
// _STATUS_TO_RPC (reference error mapping handler.go:117-127)
inline void status_to_rpc(int status, int* code, const char** msg) {
  switch (status) {
    case E_PARSE: *code = -32700; *msg = "parse error"; break;
    case E_INVALID_REQUEST: *code = -32600; *msg = "invalid request"; break;
    case E_METHOD_NOT_FOUND: *code = -32601; *msg = "tool not found"; break;
    case E_INVALID_PARAMS: *code = -32602; *msg = "invalid params"; break;
    case E_LIMIT: *code = -32602; *msg = "argument limits exceeded"; break;
    default: *code = -32603; *msg = "internal error"; break;
  }
}

// `id` is the raw JSON-RPC id token of the request; nullptr prints null
inline void envelope_head(std::string& out, const char* id, size_t id_len) {
  out.clear();
  out += "{\"jsonrpc\":\"2.0\",\"id\":";
  if (id)
    out.append(id, id_len);
  else
    out += "null";
}

// {"jsonrpc":"2.0","id":ID,"error":{"code":C,"message":"M"}}
inline void rpc_error_envelope(std::string& out, const char* id, size_t id_len,
                               int code, const char* msg) {
  envelope_head(out, id, id_len);
  out += ",\"error\":{\"code\":";
  out += std::to_string(code);
  out += ",\"message\":\"";
  json_escape_append(out, msg, strlen(msg));
  out += "\"}}";
}

// gRPC failure -> isError tool result with HTTP 200 (handler.go:252-259;
// text format matches engine/batch.py _host_slot)
inline void grpc_error_envelope(std::string& out, const char* id,
                                size_t id_len, int status,
                                const char* detail) {
  envelope_head(out, id, id_len);
  out += ",\"result\":{\"content\":[{\"type\":\"text\",\"text\":\"gRPC error ";
  out += grpc_status_name(status);
  out += ": ";
  json_escape_append(out, detail, strlen(detail));
  out += "\"}],\"isError\":true}}";
}

// Verdict on one unary reply of H2GrpcClient::invoke_raw.  status 0: the
// payload is data[off, off+len).  Otherwise a gRPC status with its text in
// `err`, which points at a literal or into the caller's `msg`.
struct GrpcReply {
  int status;
  size_t off, len;
  const char* err;
};

// parse_grpc_reply's own verdict texts (pinned by tests/test_span_host.py)
constexpr const char* GRPC_NO_STATUS = "stream closed without grpc-status";
constexpr const char* GRPC_COMPRESSED =
    "compressed gRPC response frame not supported";
constexpr const char* GRPC_TRUNCATED = "truncated gRPC frame";

// `status` is the grpc-status trailer (< 0: none arrived), `data` the DATA
// bytes of the stream, `msg` the peer's grpc-message.
inline GrpcReply parse_grpc_reply(int status, const std::string& data,
                                  const std::string& msg) {
  size_t plen = 0, poff = 0;
  bool compressed = false, truncated = false;
  if (!data.empty()) {
    if (data.size() >= 5) {
      // gRPC frame: [compressed-flag u8][len u32be][payload]
      compressed = data[0] != 0;
      uint32_t len;
      memcpy(&len, data.data() + 1, 4);
      len = ntohl(len);
      if (data.size() >= 5 + (size_t)len) {
        poff = 5;
        plen = len;
      } else {
        truncated = true;
      }
    } else {
      truncated = true;
    }
  }
  // A stream that closed without a decodable grpc-status trailer is
  // malformed (gRPC requires trailers) — never treat it as OK, even when
  // DATA arrived.
  if (status < 0)
    return {2 /*UNKNOWN*/, 0, 0,
            msg.empty() ? GRPC_NO_STATUS : msg.c_str()};
  if (status == 0 && compressed)
    return {13 /*INTERNAL*/, 0, 0, GRPC_COMPRESSED};
  if (status == 0 && truncated)
    return {13 /*INTERNAL*/, 0, 0, GRPC_TRUNCATED};
  if (status == 0) return {0, poff, plen, nullptr};
  return {status, 0, 0, msg.c_str()};
}

}  // namespace spanhost
