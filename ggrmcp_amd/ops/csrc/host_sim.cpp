// _hostsim — CPU build of the gfx950 kernels (single-lane, see host_shim.h).
//
// Purpose: (1) bit-exact CPU oracle for the device kernels so kernel
// semantics are testable in the GPU-less CI tier; (2) an ASAN/gdb-debuggable
// mirror for chasing kernel memory bugs.  The buffer/offset layout matches
// Engine::encode/decode (engine.cpp) exactly.

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#ifndef GGRMCP_HOST_SIM
#error "compile with -DGGRMCP_HOST_SIM -DWAVE=1"
#endif

#include "json2pb.hip"
#include "pb2json.hip"
#include "span_host.h"

SimDim3 threadIdx, blockIdx, blockDim, gridDim;

namespace py = pybind11;

namespace {

struct Blob {
  std::string data;
  const uint8_t* ptr() const { return (const uint8_t*)data.data(); }
};

}  // namespace

class HostEngine {
 public:
  HostEngine(py::bytes msg_table, py::bytes field_table, py::bytes enum_table,
             py::bytes enum_values, py::bytes tool_table, py::bytes name_blob,
             int n_msgs, int n_tools, py::bytes type_table)
      : msgs_{msg_table}, fields_{field_table}, enums_{enum_table},
        enum_vals_{enum_values}, tools_{tool_table}, names_{name_blob},
        types_{type_table} {
    t_.msgs = (const MsgEntry*)msgs_.ptr();
    t_.fields = (const FieldEntry*)fields_.ptr();
    t_.enums = (const EnumEntry*)enums_.ptr();
    t_.enum_vals = (const EnumValueEntry*)enum_vals_.ptr();
    t_.tools = (const ToolEntry*)tools_.ptr();
    t_.names = names_.ptr();
    t_.n_msgs = n_msgs;
    t_.n_tools = n_tools;
    t_.types = (const TypeEntry*)types_.ptr();
    t_.n_types = (int32_t)(types_.data.size() / sizeof(TypeEntry));
  }

  py::tuple encode(py::buffer data, py::array_t<uint32_t> in_off,
                   py::array_t<uint32_t> pb_off, py::object msg_idx, int mode,
                   uint32_t max_depth, uint32_t max_string, uint32_t max_args,
                   int enforce) {
    py::buffer_info din = data.request();
    auto in_off_v = in_off.unchecked<1>();
    auto pb_off_v = pb_off.unchecked<1>();
    int n = (int)in_off_v.shape(0) - 1;
    size_t pb_bytes = pb_off_v(n);
    std::vector<uint8_t> pb(pb_bytes, 0);
    std::vector<SlotResult> results(n);
    std::vector<uint8_t> ids((size_t)n * ID_SLOT_BYTES, 0);
    const int32_t* mi = nullptr;
    py::array_t<int32_t> mi_arr;
    if (!msg_idx.is_none()) {
      mi_arr = msg_idx.cast<py::array_t<int32_t>>();
      mi = mi_arr.data();
    }
    Limits lim{max_depth, max_string, max_args, (uint32_t)enforce};
    run_json2pb((const uint8_t*)din.ptr, in_off.data(), pb.data(),
                pb_off.data(), results.data(), ids.data(), mi, n, mode, lim);
    last_results_ = results;
    last_ids_ = ids;
    py::array_t<uint8_t> res({(py::ssize_t)(n * sizeof(SlotResult))});
    std::memcpy(res.mutable_data(), results.data(), n * sizeof(SlotResult));
    return py::make_tuple(res, py::bytes((const char*)pb.data(), pb.size()));
  }

  py::tuple decode(py::buffer data, py::array_t<uint32_t> resp_off,
                   py::array_t<uint32_t> scratch_off,
                   py::array_t<uint32_t> final_off, py::array_t<int32_t> msg_idx,
                   py::object skip, int mode) {
    return decode_impl(data, resp_off, scratch_off, final_off, msg_idx, skip,
                       mode, false);
  }

  // decode, then the workgroup kernel's host driver (wg_decode_host) over
  // the slots whose skip tag is 2, as Engine::launch_decode does: kind 0 only
  py::tuple decode_wg(py::buffer data, py::array_t<uint32_t> resp_off,
                      py::array_t<uint32_t> scratch_off,
                      py::array_t<uint32_t> final_off,
                      py::array_t<int32_t> msg_idx, py::object skip, int mode) {
    if ((mode & DM_KIND) != 0 || skip.is_none())
      throw std::runtime_error("decode_wg: envelope mode with a skip array");
    return decode_impl(data, resp_off, scratch_off, final_off, msg_idx, skip,
                       mode, true);
  }

  // k_pb2json_wg's scanner alone (pb2json_wg.h wgd_scan), as the device
  // extension's probe: [(start, end, kind)], empty for the classic pass
  std::vector<std::array<uint32_t, 3>> wg_scan_probe(const std::string& wire,
                                                     int msg_idx, int mode) {
    if (msg_idx < 0 || msg_idx >= t_.n_msgs)
      throw std::invalid_argument("wg_scan_probe: msg_idx");
    // exact-size copy of the wire: the scanner reads no byte past it
    std::vector<uint8_t> in(wire.begin(), wire.end());
    std::vector<uint32_t> out(WG_SCAN_PROBE_WORDS);
    auto S = std::make_unique<WgDecState>();
    WgDecReq q{};
    q.pb = in.data();
    q.wire_len = (uint32_t)in.size();
    q.msg_idx = msg_idx;
    q.flags = mode & (DM_UNPOPULATED | DM_STRUCTURED);
    threadIdx.x = 0;
    wgd_scan(*S, q, t_);
    wgd_scan_dump(*S, out.data());
    return wgd_scan_items(out.data());
  }

  // k_json2pb_wg's packed-array chunk items alone (json2pb.hip
  // wg_pack_chunks_host): the element text of one array of the message's
  // field_idx-th field, cut at the comma offsets `cuts` -> (status, wire)
  py::tuple encode_packed_chunks(int msg_idx, int field_idx,
                                 const std::string& text,
                                 const std::vector<uint32_t>& cuts) {
    if (msg_idx < 0 || msg_idx >= t_.n_msgs || field_idx < 0 ||
        field_idx >= (int)t_.msgs[msg_idx].field_count)
      throw std::invalid_argument("encode_packed_chunks: msg_idx / field_idx");
    const int field = (int)t_.msgs[msg_idx].field_start + field_idx;
    const FieldEntry& f = t_.fields[field];
    if (!(f.flags & F_REPEATED) || (f.flags & F_MAP) || !is_packable(f.kind))
      throw std::invalid_argument("encode_packed_chunks: not a packed array");
    std::string wire;
    int status = wg_pack_chunks_host(t_, field, (const uint8_t*)text.data(),
                                     (uint32_t)text.size(), cuts.data(),
                                     (int)cuts.size(), &wire);
    if (status < 0)
      throw std::invalid_argument("encode_packed_chunks: cuts");
    return py::make_tuple(status, py::bytes(wire));
  }

 private:
  py::tuple decode_impl(py::buffer data, py::array_t<uint32_t> resp_off,
                        py::array_t<uint32_t> scratch_off,
                        py::array_t<uint32_t> final_off,
                        py::array_t<int32_t> msg_idx, py::object skip, int mode,
                        bool wg) {
    py::buffer_info din = data.request();
    auto resp_off_v = resp_off.unchecked<1>();
    int n = (int)resp_off_v.shape(0) - 1;
    auto scratch_off_v = scratch_off.unchecked<1>();
    auto final_off_v = final_off.unchecked<1>();
    std::vector<uint8_t> scratch(scratch_off_v(n), 0);
    std::vector<uint8_t> fin(final_off_v(n), 0);
    std::vector<DecodeResult> results(n);
    const int32_t* skip_ptr = nullptr;
    py::array_t<int32_t> skip_arr;
    if (!skip.is_none()) {
      skip_arr = skip.cast<py::array_t<int32_t>>();
      skip_ptr = skip_arr.data();
    }
    run_pb2json((const uint8_t*)din.ptr, resp_off.data(), msg_idx.data(),
                (mode & DM_KIND) == 0 ? last_ids_.data() : nullptr,
                (mode & DM_KIND) == 0 ? last_results_.data() : nullptr,
                scratch.data(),
                scratch_off.data(), fin.data(), final_off.data(),
                results.data(), skip_ptr, n, mode);
    if (wg)
      wg_decode_host((const uint8_t*)din.ptr, resp_off.data(), msg_idx.data(),
                     last_ids_.data(), last_results_.data(), scratch.data(),
                     scratch_off.data(), fin.data(), final_off.data(),
                     results.data(), skip_ptr, t_, n, mode);
    if (mode & DM_REORDER) {
      // k_pb_reorder's phases over the slots left at E_UNSUPPORTED, in an
      // arena laid out as the engine's (pb_reorder.h ro_region)
      std::vector<uint8_t> arena(ro_region(resp_off_v(n), n), 0);
      reorder_host((const uint8_t*)din.ptr, resp_off.data(), msg_idx.data(),
                   (mode & DM_KIND) == 0 ? last_ids_.data() : nullptr,
                   (mode & DM_KIND) == 0 ? last_results_.data() : nullptr,
                   scratch.data(), scratch_off.data(), fin.data(),
                   final_off.data(), results.data(), skip_ptr, arena.data(),
                   t_, n, mode);
    }
    py::array_t<uint8_t> res({(py::ssize_t)(n * sizeof(DecodeResult))});
    std::memcpy(res.mutable_data(), results.data(), n * sizeof(DecodeResult));
    return py::make_tuple(res, py::bytes((const char*)fin.data(), fin.size()));
  }

  // drive the kernels one wave (= one request) at a time, WAVE=1 lanes
  void run_json2pb(const uint8_t* in, const uint32_t* in_off, uint8_t* pb,
                   const uint32_t* pb_off, SlotResult* results, uint8_t* ids,
                   const int32_t* mi, int n, int mode, Limits lim) {
    gridDim.x = (unsigned)((n + WPB - 1) / WPB);
    for (unsigned b = 0; b < gridDim.x; ++b) {
      for (int w = 0; w < WPB; ++w) {
        blockIdx.x = b;
        threadIdx.x = (unsigned)(w * WAVE);
        k_json2pb(in, in_off, pb, pb_off, results, ids, mi, t_, lim, n, mode,
                  nullptr);
      }
    }
  }
  void run_pb2json(const uint8_t* resp, const uint32_t* resp_off,
                   const int32_t* msg_idx, const uint8_t* ids,
                   const SlotResult* enc, uint8_t* scratch,
                   const uint32_t* scratch_off, uint8_t* fin,
                   const uint32_t* final_off, DecodeResult* results,
                   const int32_t* skip, int n, int mode) {
    gridDim.x = (unsigned)((n + WPB - 1) / WPB);
    for (unsigned b = 0; b < gridDim.x; ++b) {
      for (int w = 0; w < WPB; ++w) {
        blockIdx.x = b;
        threadIdx.x = (unsigned)(w * WAVE);
        k_pb2json(resp, resp_off, msg_idx, ids, enc, scratch, scratch_off, fin,
                  final_off, results, skip, t_, n, mode);
      }
    }
  }

  Blob msgs_, fields_, enums_, enum_vals_, tools_, names_, types_;
  Tables t_{};
  std::vector<SlotResult> last_results_;
  std::vector<uint8_t> last_ids_;
};

PYBIND11_MODULE(_hostsim, m) {
  m.doc() = "single-lane CPU build of the gfx950 transcode kernels";
  py::class_<HostEngine>(m, "HostEngine")
      .def(py::init<py::bytes, py::bytes, py::bytes, py::bytes, py::bytes,
                    py::bytes, int, int, py::bytes>(),
           py::arg("msg_table"), py::arg("field_table"), py::arg("enum_table"),
           py::arg("enum_values"), py::arg("tool_table"), py::arg("name_blob"),
           py::arg("n_msgs"), py::arg("n_tools"),
           py::arg("type_table") = py::bytes())
      .def("encode", &HostEngine::encode, py::arg("data"), py::arg("in_off"),
           py::arg("pb_off"), py::arg("msg_idx") = py::none(),
           py::arg("mode") = 0, py::arg("max_depth") = 10,
           py::arg("max_string") = 1024, py::arg("max_args") = 1u << 20,
           py::arg("enforce") = 1)
      .def("decode", &HostEngine::decode, py::arg("data"), py::arg("resp_off"),
           py::arg("scratch_off"), py::arg("final_off"), py::arg("msg_idx"),
           py::arg("skip") = py::none(), py::arg("mode") = 0)
      .def("decode_wg", &HostEngine::decode_wg, py::arg("data"),
           py::arg("resp_off"), py::arg("scratch_off"), py::arg("final_off"),
           py::arg("msg_idx"), py::arg("skip"), py::arg("mode") = 0)
      .def("wg_scan_probe", &HostEngine::wg_scan_probe, py::arg("wire"),
           py::arg("msg_idx"), py::arg("mode") = 0)
      .def("encode_packed_chunks", &HostEngine::encode_packed_chunks,
           py::arg("msg_idx"), py::arg("field_idx"), py::arg("text"),
           py::arg("cuts"));

  // k_json2pb_wg phase C's length backfill (json2pb.hip wg_pack_backfill)
  // for a split array of field `number` whose chunk items are `lens` bytes
  // long: (fits, the 3 bytes of the length slot)
  m.def("wg_pack_backfill", [](uint32_t number, std::vector<uint32_t> lens) {
    uint8_t item[8] = {0};  // a tag is at most 5 bytes
    bool ok = wg_pack_backfill(item, number, lens.data(), (int)lens.size());
    uint32_t head = varint_len(((uint64_t)number << 3) | W_LEN);
    return py::make_tuple(ok, py::bytes((const char*)item + head, LEN_SLOT));
  }, py::arg("number"), py::arg("lens"));
  m.attr("WG_ENC_PACK_CHUNK") = (int)WG_ENC_PACK_CHUNK;
  m.attr("WG_ENC_ITEM_PAD") = (int)WG_ENC_ITEM_PAD;

  // k_pack_out's offset arithmetic (pb2json.hip pack_partial / pack_place,
  // summed over the kernel's 256 thread indices) for a batch of out_len
  // values: (out_off[n], write[n], total) where total is what the engine
  // reads back, out_off + aligned out_len of the last slot, and the packed
  // block is used when total <= dst_cap
  m.def("pack_offsets", [](py::array_t<uint32_t> lens, uint32_t dst_cap) {
    int n = (int)lens.size();
    std::vector<DecodeResult> rs(n), packed(n);
    for (int i = 0; i < n; ++i) rs[i] = {E_OK, 0, lens.data()[i], 0};
    py::array_t<uint32_t> offs(n);
    py::array_t<bool> writes(n);
    for (int i = 0; i < n; ++i) {
      PackPlace p = pack_slot_host(rs.data(), n, i, dst_cap);
      packed[i] = rs[i];
      packed[i].out_off = offs.mutable_data()[i] = p.out_off;
      writes.mutable_data()[i] = p.write;
    }
    return py::make_tuple(offs, writes, pack_total(packed.data(), n));
  }, py::arg("lens"), py::arg("dst_cap"));

  // emit_packed_varint alone (pb2json.hip pv_probe), as the device
  // extension's probe: (status, text, element count of every window)
  m.def("packed_varint_probe", [](const std::string& kind,
                                  const std::string& body, uint32_t cap) {
    const uint32_t k = pv_probe_kind(kind.c_str());
    if (!k) throw std::invalid_argument("packed_varint_probe: kind " + kind);
    std::vector<uint8_t> in(body.begin(), body.end()), text(cap);
    std::vector<uint32_t> trace(PV_TRACE_CAP);
    uint32_t res[3] = {0, 0, 0};
    pv_probe(in.data(), (uint32_t)in.size(), k, text.data(), cap, trace.data(),
             res, 0);
    trace.resize(res[2]);
    return py::make_tuple((int)res[0],
                          py::bytes((const char*)text.data(), res[1]), trace);
  }, py::arg("kind"), py::arg("body"), py::arg("cap"));
  m.attr("PV_STRETCH") = (int)PV_STRETCH;
  m.attr("WG_DEC_PACK_CHUNK") = (int)WG_DEC_PACK_CHUNK;
  m.attr("WG_DEC_MAX_ITEMS") = (int)WG_DEC_MAX_ITEMS;

  // the native spans' pure host pieces (span_host.h), for the CPU tier
  m.def("grpc_reply", [](int status, const std::string& data,
                         const std::string& msg) {
    spanhost::GrpcReply g = spanhost::parse_grpc_reply(status, data, msg);
    return py::make_tuple(g.status, g.off, g.len,
                          g.err ? py::object(py::str(g.err)) : py::none());
  }, py::arg("status"), py::arg("data"), py::arg("msg"));
  m.def("status_to_rpc", [](int status) {
    int code;
    const char* msg;
    spanhost::status_to_rpc(status, &code, &msg);
    return py::make_tuple(code, msg);
  }, py::arg("status"));
  m.def("rpc_error_envelope", [](std::optional<std::string> id, int code,
                                 const std::string& msg) {
    std::string out;
    spanhost::rpc_error_envelope(out, id ? id->data() : nullptr,
                                 id ? id->size() : 0, code, msg.c_str());
    return py::bytes(out);
  }, py::arg("id"), py::arg("code"), py::arg("msg"));
  m.def("grpc_error_envelope", [](std::optional<std::string> id, int status,
                                  const std::string& detail) {
    std::string out;
    spanhost::grpc_error_envelope(out, id ? id->data() : nullptr,
                                  id ? id->size() : 0, status, detail.c_str());
    return py::bytes(out);
  }, py::arg("id"), py::arg("status"), py::arg("detail"));
}
