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
           py::arg("msg_idx"), py::arg("skip"), py::arg("mode") = 0);

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
