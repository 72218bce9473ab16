"""Shared protojson corpus for the CPU (hostsim) and gfx950 differential
suites, plus the lane-window sweep generators.

A plain helper module, not a conftest: ``test_protojson_surface.py``,
``test_gpu_protojson_surface.py`` and the lane-window tests import it.

The oracle is ``google.protobuf.json_format`` on the real message class of
``t.Sink`` — a "kitchen sink" schema covering the protojson surface the
four production-shaped schemas never touch (packed scalars, every map key
type, the well-known types, long bytes).

Contract (``check_*`` below):

* where the oracle raises, the kernel status must be non-zero;
* where the oracle accepts, the kernel must return status 0 and an equal
  value — unless the case carries a ``HOST`` tag, in which case the kernel
  may also hand the slot to the host with E_UNSUPPORTED/E_OVERFLOW (6/7)
  and nothing else.  A tag names a rule written down in docs/KERNELS.md
  ("Host-escape rules") and is assigned from that rule, not from what the
  kernel happened to return.
"""

from __future__ import annotations

import base64
import json
import math
import random
import struct
from typing import Any, List, NamedTuple, Optional, Sequence

from google.protobuf import json_format, message_factory
from google.protobuf.message import DecodeError

from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from ggrmcp_amd.utils.protobuild import FileBuilder
from ggrmcp_amd.utils.synthetic import synthetic_fdp

E_PARSE = 1
E_UNSUPPORTED = 6
E_OVERFLOW = 7
HOST_STATUSES = (E_UNSUPPORTED, E_OVERFLOW)

# ---- schema -----------------------------------------------------------------

SCALAR_KINDS = [
    "double", "float", "int64", "uint64", "int32", "fixed64", "fixed32",
    "bool", "uint32", "sfixed32", "sfixed64", "sint32", "sint64",
]
MAP_KEY_KINDS = [
    "int32", "int64", "uint32", "uint64", "sint32", "sint64", "fixed32",
    "fixed64", "sfixed32", "sfixed64", "bool", "string",
]
WRAPPERS = [
    ("w_double", "DoubleValue"), ("w_float", "FloatValue"),
    ("w_int64", "Int64Value"), ("w_uint64", "UInt64Value"),
    ("w_int32", "Int32Value"), ("w_uint32", "UInt32Value"),
    ("w_bool", "BoolValue"), ("w_string", "StringValue"),
    ("w_bytes", "BytesValue"),
]

# field name -> number; filled by sink_fdp() so WIRES can name fields
F = {}


def sink_fdp():
    """t.Sink: every protojson feature in one message."""
    F.clear()
    fb = FileBuilder("t/sink.proto", "t")
    fb.add_dependency(
        "google/protobuf/duration.proto", "google/protobuf/timestamp.proto",
        "google/protobuf/field_mask.proto", "google/protobuf/empty.proto",
        "google/protobuf/struct.proto", "google/protobuf/wrappers.proto")
    fb.enum("Color", [("C_ZERO", 0), ("C_ONE", 1), ("C_NEG", -1)])
    fb.message("Leaf").field("id", 1, "int32").field("tag", 2, "string").done()
    m = fb.message("Sink")
    num = [0]

    def nxt(name):
        num[0] += 1
        F[name] = num[0]
        return num[0]

    for k in SCALAR_KINDS:
        m.field(f"r_{k}", nxt(f"r_{k}"), k, repeated=True)
    m.field("r_enum", nxt("r_enum"), "enum", enum="Color", repeated=True)
    m.field("r_bytes", nxt("r_bytes"), "bytes", repeated=True)
    m.field("blob", nxt("blob"), "bytes")
    for k in MAP_KEY_KINDS:
        m.map_field(f"m_{k}", nxt(f"m_{k}"), k, "int32")
    m.map_field("m_msg", nxt("m_msg"), "string", "message", "Leaf")
    m.map_field("m_enum", nxt("m_enum"), "string", "enum", "Color")
    m.map_field("m_dbl", nxt("m_dbl"), "string", "double")
    m.map_field("m_bytes", nxt("m_bytes"), "string", "bytes")
    for name, wkt in [("dur", "Duration"), ("ts", "Timestamp"),
                      ("mask", "FieldMask"), ("empty", "Empty"),
                      ("val", "Value"), ("lst", "ListValue"),
                      ("st", "Struct")]:
        m.field(name, nxt(name), "message", message=f"google.protobuf.{wkt}")
    for name, wkt in WRAPPERS:
        m.field(name, nxt(name), "message", message=f"google.protobuf.{wkt}")
    m.field("r_dur", nxt("r_dur"), "message",
            message="google.protobuf.Duration", repeated=True)
    m.field("r_w32", nxt("r_w32"), "message",
            message="google.protobuf.Int32Value", repeated=True)
    m.field("opt_i32", nxt("opt_i32"), "int32", optional=True)
    m.field("opt_str", nxt("opt_str"), "string", optional=True)
    m.field("snake_case_field", nxt("snake_case_field"), "string")
    m.field("custom", nxt("custom"), "string", json_name="renamed")
    m.field("leaf", nxt("leaf"), "message", message="Leaf")
    m.done()
    fb.service("SinkService").method("Echo", "Sink", "Sink").done()
    return fb.build()


class Env(NamedTuple):
    engine: Any
    pool: Any
    infos: Any
    sink_cls: Any
    sink_idx: int
    inner_cls: Any
    inner_idx: int
    sink_tool: str
    wide_cls: Any
    wide_idx: int


def make_env(engine_factory) -> Env:
    """Build the pool/tables once and an engine from ``engine_factory(infos)``
    (HostSimEngine on the CPU tier, GpuEngine on the device tier)."""
    fdps = [sink_fdp(), synthetic_fdp()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    engine = engine_factory(infos)
    tool = next(n for n, mi in infos.items()
                if mi.input_descriptor.full_name == "t.Sink")
    return Env(
        engine, pool, infos,
        message_factory.GetMessageClass(pool.FindMessageTypeByName("t.Sink")),
        engine.tables.msg_index["t.Sink"],
        message_factory.GetMessageClass(pool.FindMessageTypeByName("bench.Inner")),
        engine.tables.msg_index["bench.Inner"],
        tool,
        message_factory.GetMessageClass(pool.FindMessageTypeByName("bench.Wide64")),
        engine.tables.msg_index["bench.Wide64"],
    )


# ---- cases ------------------------------------------------------------------

class Case(NamedTuple):
    id: str
    data: Any              # JSON text (ACCEPT/REJECT/PY_LAX) or wire bytes
    host: Optional[str] = None   # HOST tag: the KERNELS.md rule that applies


def _j(obj) -> str:
    return json.dumps(obj, ensure_ascii=False)


_I32 = (-2**31, 2**31 - 1)
_I64 = (-2**63, 2**63 - 1)
_U32 = (0, 2**32 - 1)
_U64 = (0, 2**64 - 1)
INT_RANGES = {
    "int32": _I32, "sint32": _I32, "sfixed32": _I32,
    "int64": _I64, "sint64": _I64, "sfixed64": _I64,
    "uint32": _U32, "fixed32": _U32, "uint64": _U64, "fixed64": _U64,
}


def _camel(name: str) -> str:
    parts = name.split("_")
    return parts[0] + "".join(p.capitalize() for p in parts[1:])


def _b64(n: int, seed: int = 0) -> bytes:
    return bytes((i * 37 + seed * 11 + 5) & 0xFF for i in range(n))


def _accept_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda i, d, host=None: c.append(Case(i, d, host))  # noqa: E731
    # integer extremes per width, as numbers and as strings
    for kind, (lo, hi) in INT_RANGES.items():
        key = _camel(f"r_{kind}")
        add(f"int-ext-num-{kind}", _j({key: [lo, hi, 0, 1]}))
        add(f"int-ext-str-{kind}", _j({key: [str(lo), str(hi), "0", "7"]}))
    # float spellings of integers
    add("int-as-1.0", '{"rInt32":[1.0,-5.0,1e2,1.5e1],"rUint64":[1e2,2.0]}')
    add("int64-as-1.0", '{"rInt64":[1.0,-3e2],"rSint32":[2.0],"rFixed32":[4e0]}')
    # floating point
    add("dbl-plain", '{"rDouble":[0.1,-0.0,1.5,-2.25e10,1e-7,123456789.125]}')
    add("dbl-nonfinite", '{"rDouble":["NaN","Infinity","-Infinity"]}')
    add("dbl-strings", '{"rDouble":["1.5","-2e3"]}')
    add("dbl-denormal", '{"rDouble":[5e-324,2.2250738585072014e-308]}',
        host="near-denormal doubles take the host path")
    add("dbl-max", '{"rDouble":[1.7976931348623157e308,-1.7976931348623157e308]}',
        host="near-DBL_MAX doubles take the host path")
    add("dbl-long-mantissa", '{"rDouble":[0.1000000000000000055511151231257827]}',
        host="mantissas over 19 significant digits take the host path")
    add("flt-plain", '{"rFloat":[0.1,-0.0,1.5,16777217,1e-7,3.25e10]}')
    # FLT_MAX spelled with its exact double value: json_format refuses the
    # shortest float32 text 3.4028235e+38 (it compares as a double)
    add("flt-extremes", '{"rFloat":[3.4028234663852886e38,-3.4028234663852886e38,'
                        '1.17549435e-38,1e-45]}')
    add("flt-nonfinite", '{"rFloat":["NaN","Infinity","-Infinity"]}')
    add("bool-list", '{"rBool":[true,false,true]}')
    # arrays: empty and long (length slot > 127)
    add("arrays-empty", _j({_camel(f"r_{k}"): [] for k in SCALAR_KINDS}
                           | {"rEnum": [], "rBytes": [], "rDur": [], "rW32": []}))
    add("packed-600-int32", _j({"rInt32": [(i * 7919) % 100003 - 50000 for i in range(600)]}))
    add("packed-600-sint64", _j({"rSint64": [str((-1) ** i * (i << 40)) for i in range(600)]}))
    add("packed-600-double", _j({"rDouble": [i / 8 for i in range(600)]}))
    add("packed-600-bool", _j({"rBool": [i % 3 == 0 for i in range(600)]}))
    add("packed-600-fixed32", _j({"rFixed32": [(i * 2654435761) % 2**32 for i in range(600)]}))
    add("packed-600-float", _j({"rFloat": [i / 4 for i in range(600)]}))
    # enums
    add("enum-list", '{"rEnum":["C_NEG",-1,0,"C_ONE",1,"C_ZERO"]}')
    add("enum-unknown-number", '{"rEnum":[7,-9]}')
    # bytes
    add("b64-std", '{"blob":"+/8="}')
    add("b64-url", '{"blob":"-_8="}')
    add("b64-unpadded-2", '{"blob":"+/8"}')
    add("b64-unpadded-1", '{"blob":"AA"}')
    add("b64-padded-1", '{"blob":"AA=="}')
    add("b64-empty", '{"blob":""}')
    add("b64-280", _j({"blob": base64.b64encode(_b64(210)).decode()}))
    add("b64-281-unpadded", _j({"blob": base64.b64encode(_b64(211, 1)).decode().rstrip("=")}))
    add("b64-list", _j({"rBytes": ["", "AA", "AAE=", "AAEC", "-_-_", "+/+/",
                                    base64.b64encode(_b64(100, 2)).decode()]}))
    # maps: every key type at its extremes
    for kind in MAP_KEY_KINDS:
        key = _camel(f"m_{kind}")
        if kind == "bool":
            add("map-key-bool", _j({key: {"true": 1, "false": 0}}))
        elif kind == "string":
            add("map-key-string", _j({key: {"": 1, "k": 2, "é": 3, "中😀": -4}}))
            add("map-key-string-escaped", _j({key: {'q"\\': 3, "t\n": 1}}),
                host="escaped (backslash) map keys take the host path")
        else:
            lo, hi = INT_RANGES[kind]
            add(f"map-key-{kind}", _j({key: {str(lo): -1, str(hi): 1, "0": 0, "5": 2**31 - 1}}))
    add("map-val-msg", '{"mMsg":{"a":{"id":1,"tag":"x"},"b":{},"":{"tag":"e"}}}')
    add("map-val-enum", '{"mEnum":{"a":"C_NEG","b":1,"c":"C_ZERO","d":-1}}')
    add("map-val-double", '{"mDbl":{"a":1.5,"b":"NaN","c":-0.0,"d":"-Infinity"}}')
    add("map-val-bytes", '{"mBytes":{"a":"AAEC","b":"","c":"-_8"}}')
    add("map-empty", '{"mString":{},"mInt32":{},"mMsg":{}}')
    # Duration
    for i, d in enumerate(["0s", "315576000000s", "-315576000000s", "1.5s",
                           "1.000001s", "1.000000001s", "-0.5s", "3.000s",
                           "-315576000000.999999999s", "315576000000.999999999s",
                           "0.000000001s", "-0.000000001s", "12.120s"]):
        add(f"dur-{i}-{d}", _j({"dur": d}))
    add("dur-list", _j({"rDur": ["0s", "1.5s", "-315576000000s", "0.000001s", "7s"]}))
    # Timestamp
    for i, t in enumerate(["0001-01-01T00:00:00Z",
                           "9999-12-31T23:59:59.999999999Z",
                           "1970-01-01T00:00:00Z",
                           "2023-11-14T22:13:20.123Z",
                           "2023-11-14T22:13:20.123456Z",
                           "2023-11-14T22:13:20.123456789Z",
                           "2024-02-29T12:00:00Z",
                           "2000-02-29T23:59:59Z",
                           "1969-12-31T23:59:59.5Z",
                           "2023-11-14T22:13:20+05:30",
                           "2023-11-14T22:13:20.25-08:00",
                           "1600-03-01T00:00:00Z"]):
        add(f"ts-{i}-{t}", _j({"ts": t}))
    # FieldMask
    add("mask-empty", '{"mask":""}')
    add("mask-single", '{"mask":"foo"}')
    add("mask-nested", '{"mask":"foo.barBaz,quxQuux.a.bC,z"}')
    # Value / ListValue / Struct
    add("val-null", '{"val":null}')
    add("val-number", '{"val":1.5}')
    add("val-int", '{"val":-7}')
    add("val-string", '{"val":"s\\"q\\n"}')
    add("val-bool", '{"val":true}')
    add("val-list", '{"val":[1,"a",null,false,[],{}]}')
    add("val-nested", '{"val":{"a":{"b":{"c":[1,{"d":null}]}}}}')
    add("lst-nested", '{"lst":[1,[2,[3,"x"]],{"k":[null]}]}')
    add("lst-empty", '{"lst":[]}')
    add("st-nested", '{"st":{"a":{"b":{"c":1.25}},"e":"","":true}}')
    add("st-empty", '{"st":{}}')
    add("empty", '{"empty":{}}')
    # wrappers
    add("wrappers-zero", '{"wDouble":0,"wFloat":0,"wInt64":"0","wUint64":"0",'
                         '"wInt32":0,"wUint32":0,"wBool":false,"wString":"","wBytes":""}')
    add("wrappers-values", '{"wDouble":-1.5,"wFloat":0.1,"wInt64":"-9223372036854775808",'
                           '"wUint64":"18446744073709551615","wInt32":-2147483648,'
                           '"wUint32":4294967295,"wBool":true,"wString":"é\\"","wBytes":"AAE="}')
    add("wrappers-nonfinite", '{"wDouble":"NaN","wFloat":"-Infinity"}')
    add("wrappers-list", '{"rW32":[0,1,-1,2147483647]}')
    add("nulls", '{"wInt32":null,"wString":null,"dur":null,"ts":null,"rInt32":null,'
                 '"mString":null,"leaf":null,"blob":null,"optI32":null,"st":null}')
    # names and presence
    add("name-proto", '{"snake_case_field":"a","r_int32":[1],"opt_i32":3}')
    add("name-json", '{"snakeCaseField":"a","rInt32":[1],"optI32":3}')
    add("name-custom-json", '{"renamed":"x"}')
    add("name-custom-proto", '{"custom":"x"}')
    add("optional-zero", '{"optI32":0,"optStr":""}')
    add("optional-set", '{"optI32":-1,"optStr":"s"}')
    add("leaf", '{"leaf":{"id":5,"tag":"t"}}')
    add("leaf-empty", '{"leaf":{}}')
    add("empty-object", '{}')
    return c


def _reject_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda i, d: c.append(Case(i, d))  # noqa: E731
    add("flt-overflow-repeated", '{"rFloat":[1e39]}')
    add("flt-overflow-repeated-neg", '{"rFloat":[1.0,-1e39]}')
    add("flt-overflow-wrapper", '{"wFloat":1e39}')
    add("flt-overflow-double-repeated", '{"rFloat":[1e400]}')
    add("flt-overflow-double-wrapper", '{"wFloat":-1e400}')
    add("dbl-overflow-wrapper", '{"wDouble":1e400}')
    add("dur-no-leading-digit", '{"dur":".5s"}')
    add("dur-neg-no-leading-digit", '{"dur":"-.5s"}')
    add("dbl-overflow-repeated", '{"rDouble":[1e400]}')
    add("dbl-overflow-map", '{"mDbl":{"a":-1e400}}')
    add("enum-number-over", '{"rEnum":[2147483648]}')
    add("map-key-bool-prefix", '{"mBool":{"txyz":1}}')
    add("map-key-fixed32-over", '{"mFixed32":{"4294967296":1}}')
    add("map-key-sint32-under", '{"mSint32":{"-2147483649":1}}')
    add("ts-offset-nondigit", '{"ts":"2023-01-01T00:00:00+0a:00"}')
    add("ts-hour24", '{"ts":"2023-01-01T24:00:00Z"}')

    add("b64-len1", '{"blob":"A"}')
    add("b64-three-pads", '{"blob":"A==="}')
    add("b64-len5", '{"blob":"AAAAA"}')
    add("b64-list-len1", '{"rBytes":["AAAA","A"]}')
    add("mask-underscore", '{"mask":"a_b"}')
    add("mask-underscore-nested", '{"mask":"foo.a_b"}')
    add("ts-feb30", '{"ts":"2023-02-30T00:00:00Z"}')
    add("ts-lowercase", '{"ts":"2023-01-01t00:00:00z"}')
    add("ts-lower-t", '{"ts":"2023-01-01t00:00:00Z"}')
    add("ts-lower-z", '{"ts":"2023-01-01T00:00:00z"}')
    add("ts-feb29-nonleap", '{"ts":"2023-02-29T00:00:00Z"}')
    add("ts-feb29-1900", '{"ts":"1900-02-29T00:00:00Z"}')
    add("ts-apr31", '{"ts":"2023-04-31T00:00:00Z"}')
    add("ts-day0", '{"ts":"2023-04-00T00:00:00Z"}')
    add("ts-month13", '{"ts":"2023-13-01T00:00:00Z"}')
    add("ts-year0", '{"ts":"0000-12-31T23:59:59Z"}')
    add("ts-no-zone", '{"ts":"2023-01-01T00:00:00"}')
    add("ts-10-digits", '{"ts":"2023-01-01T00:00:00.0000000001Z"}')
    for kind, (lo, hi) in INT_RANGES.items():
        key = _camel(f"r_{kind}")
        add(f"int-over-{kind}", _j({key: [hi + 1]}))
        add(f"int-over-str-{kind}", _j({key: [str(hi + 1)]}))
        add(f"int-under-{kind}", _j({key: [lo - 1]}))
        add(f"int-frac-{kind}", '{"%s":[1.5]}' % key)
    add("uint32-negative", '{"rUint32":[-1]}')
    add("uint64-negative-str", '{"rUint64":["-1"]}')
    add("fixed64-negative", '{"rFixed64":[-5]}')
    add("wrapper-int32-over", '{"wInt32":2147483648}')
    add("wrapper-uint32-neg", '{"wUint32":-1}')
    add("map-key-nonnumeric", '{"mInt32":{"x":1}}')
    add("map-key-fraction", '{"mInt32":{"1.5":1}}')
    add("map-key-over", '{"mInt32":{"2147483648":1}}')
    add("map-key-uint-neg", '{"mUint32":{"-1":1}}')
    add("map-key-bool-caps", '{"mBool":{"True":1}}')
    add("map-key-bool-num", '{"mBool":{"1":1}}')
    add("map-key-u64-over", '{"mUint64":{"18446744073709551616":1}}')
    add("map-val-over", '{"mString":{"k":2147483648}}')
    add("enum-bad-name", '{"rEnum":["NOPE"]}')
    add("enum-bad-name-map", '{"mEnum":{"a":"c_one"}}')
    add("dur-no-suffix", '{"dur":"1"}')
    add("dur-over", '{"dur":"315576000001s"}')
    add("dur-under", '{"dur":"-315576000001s"}')
    add("dur-empty", '{"dur":""}')
    add("dur-number", '{"dur":1}')
    add("int-ws-lead", '{"rInt32":[" 1"]}')
    add("int-ws-trail", '{"rInt32":["1 "]}')
    add("int-ws-mid", '{"rInt64":["1 2"]}')
    add("uint-ws", '{"rUint64":[" 5"]}')
    add("map-key-ws", '{"mInt32":{" 1":1}}')
    add("unknown-field", '{"nope":1}')
    add("bool-string-caps", '{"rBool":["True"]}')
    add("string-for-message", '{"leaf":"x"}')
    add("array-for-scalar", '{"optI32":[1]}')
    add("scalar-for-array", '{"rInt32":1}')
    add("null-in-array", '{"rInt32":[null]}')
    return c


# Spellings json_format (Python) accepts but Go protojson — the gateway this
# project mirrors — rejects.  Only "kernel status non-zero" is asserted.
#  * Duration: Go's parseDuration (well_known_types.go) admits only
#    ^-?[0-9]+(\.[0-9]{1,9})?s$ — no inner whitespace, no leading '+'.
#  * bytes: Go unmarshalBytes uses encoding/base64 strict decoding, which
#    rejects any character outside the alphabet, whitespace included.
#  Direct variants: Python also rounds a tenth fraction digit away instead
#  of refusing it, takes "1.s", skips ANY non-alphabet byte ('*', or '='
#  before the end), not just a space, and re-pads "AA=" itself.
PY_LAX = [
    Case("dur-inner-space", '{"dur":"1.5 s"}'),
    Case("dur-plus-sign", '{"dur":"+1s"}'),
    Case("dur-10-digits", '{"dur":"1.0000000001s"}'),
    Case("b64-inner-space", '{"blob":"A A="}'),
    Case("b64-bad-char", '{"blob":"AA*A"}'),
    Case("b64-pad-mid", '{"blob":"AA=A"}'),
    Case("b64-one-pad-short", '{"blob":"AA="}'),
    Case("dur-no-fraction-digits", '{"dur":"1.s"}'),
]

# Two more spellings of the same kind outside Duration and bytes: Python
# accepts them, Go refuses, the kernels follow Go.
#  * Timestamp: Go parses with time.RFC3339Nano, whose numeric offset is
#    bounded (hour <= 23, minute <= 59).
#  * FieldMask: Go splits on ',' and requires every path to be a valid
#    protoreflect.FullName — no empty path and no empty name segment.
GO_STRICT = [
    Case("ts-offset-out-of-range", '{"ts":"2023-01-01T00:00:00+99:99"}'),
    Case("ts-offset-minute-60", '{"ts":"2023-01-01T00:00:00-01:60"}'),
    Case("mask-empty-segment", '{"mask":"a..b"}'),
    Case("mask-leading-dot", '{"mask":".a"}'),
    Case("mask-empty-path", '{"mask":"a,,b"}'),
    Case("mask-trailing-comma", '{"mask":"a,"}'),
]


# ---- hand-assembled wire ----------------------------------------------------

def vi(n: int) -> bytes:
    n &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def tag(field: int, wt: int) -> bytes:
    return vi(field << 3 | wt)


def ld(field: int, body: bytes) -> bytes:
    return tag(field, 2) + vi(len(body)) + body


# HOST-or-equal: see docs/PARITY.md and the KERNELS.md rule of the same words
DUP_KEYS = "a map key repeated on the wire may take the host path"


def _zz(n: int) -> int:
    return (n << 1) ^ (n >> 63)


def _wire_cases() -> List[Case]:
    sink_fdp()  # fill F
    c: List[Case] = []
    add = lambda i, d, host=None: c.append(Case(i, d, host))  # noqa: E731
    REOCCUR = "out-of-order or re-occurring fields take the host path"
    DUP = DUP_KEYS
    f = F
    # packed vs unpacked
    add("unpacked-int32", b"".join(tag(f["r_int32"], 0) + vi(v) for v in (1, 2, 300)))
    add("unpacked-double", b"".join(tag(f["r_double"], 1) + struct.pack("<d", v)
                                    for v in (1.5, -2.0)))
    add("unpacked-fixed32", tag(f["r_fixed32"], 5) + b"\x01\x00\x00\x00")
    add("packed-mixed-runs",
        ld(f["r_int32"], vi(1) + vi(2)) + tag(f["r_int32"], 0) + vi(3)
        + ld(f["r_int32"], vi(4)))
    add("packed-empty-run", ld(f["r_int32"], b""))
    add("packed-empty-then-data", ld(f["r_int32"], b"") + ld(f["r_int32"], vi(9)))
    add("packed-two-fields", ld(f["r_int32"], vi(1)) + ld(f["r_bool"], b"\x01\x00"))
    # varint edge encodings
    add("int32-negative-10-byte", tag(f["opt_i32"], 0) + vi(-1))
    add("int32-min", tag(f["opt_i32"], 0) + vi(-2**31))
    add("int32-high-bits", tag(f["opt_i32"], 0) + vi((1 << 32) | 5))
    add("int32-packed-high-bits", ld(f["r_int32"], vi((7 << 32) | 0xFFFFFFFF) + vi(-5)))
    add("varint-non-minimal", tag(f["opt_i32"], 0) + b"\x81\x80\x00")
    add("varint-non-minimal-tag", _nonminimal_tag(f["opt_i32"], 0) + vi(4))
    add("uint32-high-bits", ld(f["r_uint32"], vi((1 << 35) | 9)))
    add("uint64-max", ld(f["r_uint64"], vi(2**64 - 1)))
    add("int64-min", ld(f["r_int64"], vi(-2**63) + vi(2**63 - 1)))
    # enums
    add("enum-unknown", ld(f["r_enum"], vi(7)))
    add("enum-negative", ld(f["r_enum"], vi(-1) + vi(0) + vi(1)))
    add("enum-unknown-negative-unpacked", tag(f["r_enum"], 0) + vi(-9))
    # map entries
    ms, mi, mm, me = f["m_string"], f["m_int32"], f["m_msg"], f["m_enum"]
    add("map-key-missing", ld(ms, tag(2, 0) + vi(5)))
    add("map-value-missing", ld(ms, ld(1, b"k")))
    add("map-both-missing", ld(ms, b""))
    add("map-value-before-key", ld(ms, tag(2, 0) + vi(5) + ld(1, b"k")))
    add("map-int-key-missing", ld(mi, tag(2, 0) + vi(5)))
    add("map-int-value-before-key", ld(mi, tag(2, 0) + vi(5) + tag(1, 0) + vi(-3)))
    add("map-msg-value-missing", ld(mm, ld(1, b"k")))
    add("map-enum-value-missing", ld(me, ld(1, b"k")))
    add("map-bool-keys", ld(f["m_bool"], tag(1, 0) + vi(1) + tag(2, 0) + vi(1))
        + ld(f["m_bool"], tag(2, 0) + vi(2)))
    add("map-sint-key", ld(f["m_sint32"], tag(1, 0) + vi(_zz(-2**31)) + tag(2, 0) + vi(1)))
    add("map-fixed64-key", ld(f["m_fixed64"], tag(1, 1) + b"\xff" * 8 + tag(2, 0) + vi(1)))
    add("map-sfixed32-key", ld(f["m_sfixed32"], tag(1, 5) + b"\xff" * 4 + tag(2, 0) + vi(1)))
    add("map-duplicate-keys",
        ld(ms, ld(1, b"k") + tag(2, 0) + vi(1)) + ld(ms, ld(1, b"k") + tag(2, 0) + vi(2)),
        host=DUP)
    add("map-duplicate-keys-apart",
        ld(ms, ld(1, b"k") + tag(2, 0) + vi(1)) + ld(ms, ld(1, b"j") + tag(2, 0) + vi(3))
        + ld(ms, ld(1, b"k") + tag(2, 0) + vi(2)), host=DUP)
    add("map-duplicate-int-keys",
        ld(mi, tag(1, 0) + vi(4) + tag(2, 0) + vi(1)) + ld(mi, tag(1, 0) + vi(4) + tag(2, 0) + vi(2)),
        host=DUP)
    add("map-distinct-keys",
        ld(ms, ld(1, b"k") + tag(2, 0) + vi(1)) + ld(ms, ld(1, b"kk") + tag(2, 0) + vi(2)))
    # unknown fields of every wire type
    U = 1000
    add("unknown-varint", tag(U, 0) + vi(99) + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-fixed64", tag(U, 1) + b"\x01" * 8 + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-len", ld(U, b"abc") + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-fixed32", tag(U, 5) + b"\x01" * 4 + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-group", tag(U, 3) + tag(1, 0) + vi(1) + ld(2, b"x") + tag(U, 4)
        + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-nested-group", tag(U, 3) + tag(U + 1, 3) + tag(U + 1, 4) + tag(U, 4)
        + tag(f["opt_i32"], 0) + vi(1))
    add("unknown-in-leaf", ld(f["leaf"], tag(1, 0) + vi(3) + tag(9, 0) + vi(1)))
    add("unknown-low-number-first", tag(f["opt_i32"], 0) + vi(1) + ld(U, b""))
    # wire-type mismatch on known fields (treated as unknown)
    add("mismatch-int-as-fixed32", tag(f["opt_i32"], 5) + b"\x01\x00\x00\x00")
    add("mismatch-string-as-varint", tag(f["opt_str"], 0) + vi(5))
    add("mismatch-message-as-varint", tag(f["leaf"], 0) + vi(5))
    add("mismatch-double-as-fixed32", tag(f["r_double"], 5) + b"\x00\x00\x80\x3f")
    # re-occurring fields
    add("dup-singular-scalar", tag(f["opt_i32"], 0) + vi(1) + tag(f["opt_i32"], 0) + vi(2),
        host=REOCCUR)
    add("dup-singular-string", ld(f["opt_str"], b"a") + ld(f["opt_str"], b"b"),
        host=REOCCUR)
    add("message-split", ld(f["leaf"], tag(1, 0) + vi(1)) + ld(f["leaf"], ld(2, b"x")),
        host=REOCCUR)
    add("fields-out-of-order", ld(f["opt_str"], b"a") + tag(f["opt_i32"], 0) + vi(1),
        host=REOCCUR)
    add("repeated-interleaved",
        ld(f["r_int32"], vi(1)) + tag(f["opt_i32"], 0) + vi(1) + ld(f["r_int32"], vi(2)),
        host=REOCCUR)
    # wrappers
    add("wrappers-empty-bodies", b"".join(ld(f[n], b"") for n, _ in WRAPPERS))
    add("wrappers-explicit-zero", ld(f["w_int32"], tag(1, 0) + vi(0))
        + ld(f["w_string"], ld(1, b"")))
    add("wrapper-list-empty-bodies", ld(f["r_w32"], b"") + ld(f["r_w32"], tag(1, 0) + vi(5)))
    add("empty-bodies-wkt", ld(f["dur"], b"") + ld(f["ts"], b"") + ld(f["mask"], b"")
        + ld(f["empty"], b"") + ld(f["val"], b"") + ld(f["lst"], b"") + ld(f["st"], b""))
    # bools
    add("bool-varint-2", ld(f["r_bool"], b"\x02\x80\x01\x00\x01"))
    add("bool-varint-wide", ld(f["r_bool"], vi(1 << 40) + vi(2**64 - 1)))
    # zigzag and fixed widths
    add("zigzag32-extremes", ld(f["r_sint32"], vi(0xFFFFFFFF) + vi(0xFFFFFFFE) + vi(1) + vi(0)))
    add("zigzag64-extremes", ld(f["r_sint64"], vi(2**64 - 1) + vi(2**64 - 2) + vi(1)))
    add("fixed32-all-ones", ld(f["r_fixed32"], b"\xff" * 4) + ld(f["r_sfixed32"], b"\xff" * 4))
    add("fixed64-all-ones", ld(f["r_fixed64"], b"\xff" * 8) + ld(f["r_sfixed64"], b"\xff" * 8))
    add("float-all-ones", ld(f["r_float"], b"\xff" * 4))
    add("double-all-ones", ld(f["r_double"], b"\xff" * 8))
    add("double-neg-zero", ld(f["r_double"], struct.pack("<d", -0.0))
        + ld(f["r_float"], struct.pack("<f", -0.0)))
    # strings and bytes
    add("bytes-long", ld(f["blob"], _b64(211)))
    add("string-escapes", ld(f["opt_str"], 'a"\\\n\x01é中😀'.encode()))
    add("string-invalid-utf8", ld(f["opt_str"], b"a\x80"))
    # truncation
    add("trunc-len", tag(f["opt_str"], 2) + vi(10) + b"abc")
    add("trunc-packed-fixed32", ld(f["r_fixed32"], b"\x01\x00\x00\x00\x02\x00"))
    add("trunc-packed-double", ld(f["r_double"], b"\x00" * 12))
    add("trunc-varint", tag(f["opt_i32"], 0) + b"\x80")
    add("trunc-tag", b"\x80")
    add("len-over-32-bits", tag(f["m_string"], 2) + vi(2**32 + 3) + ld(1, b"k"))
    add("len-over-32-bits-packed", tag(f["r_int32"], 2) + vi(2**32 + 1) + vi(5))
    U_ = 1000
    for name, n in (("2^64-k", 2**64 - 12), ("2^64-1", 2**64 - 1),
                    ("2^32+small", 2**32 + 2), ("2^63", 2**63)):
        # unknown field: the cursor must not move back onto the same tag
        add(f"len-wrap-unknown-{name}", tag(U_, 2) + vi(n))
        add(f"len-wrap-unknown-{name}-tail", tag(U_, 2) + vi(n) + b"ab")
        add(f"len-wrap-in-group-{name}", tag(U_, 3) + tag(1, 2) + vi(n) + tag(U_, 4))
        add(f"len-wrap-mismatch-{name}", tag(f["opt_i32"], 2) + vi(n) + b"ab")
        add(f"len-wrap-string-{name}", tag(f["opt_str"], 2) + vi(n) + b"ab")
        add(f"len-wrap-in-entry-{name}", ld(f["m_string"], tag(3, 2) + vi(n)))
    # the reviewer-style exact loops: length = 2^64 - (tag + 10 varint bytes)
    add("len-wrap-back-to-tag", bytes.fromhex("c23ef4ffffffffffffffff01"))
    add("len-wrap-back-to-tag-in-group", bytes.fromhex("c33e0af5ffffffffffffffff01c43e"))
    add("group-end-number-differs", tag(1000, 3) + tag(1001, 4))
    add("group-interleaved", tag(1000, 3) + tag(1001, 3) + tag(1000, 4) + tag(1001, 4))
    add("group-nested-matched", tag(1000, 3) + tag(1001, 3) + tag(1, 0) + vi(1)
        + tag(1001, 4) + tag(1000, 4) + tag(f["opt_i32"], 0) + vi(2))
    add("group-inner-end-differs", tag(1000, 3) + tag(1001, 3) + tag(1002, 4) + tag(1000, 4))
    add("group-nested-9-deep", b"".join(tag(1000 + i, 3) for i in range(9))
        + b"".join(tag(1000 + i, 4) for i in reversed(range(9)))
        + tag(f["opt_i32"], 0) + vi(2),
        host="unknown groups nested more than 8 deep take the host path")
    add("end-group-alone", tag(1000, 4))
    add("group-unterminated", tag(1000, 3) + tag(1, 0) + vi(1))
    add("trunc-nested", ld(f["leaf"], tag(2, 2) + vi(5) + b"ab"))
    add("trunc-fixed64", tag(f["r_double"], 1) + b"\x00" * 5)
    add("varint-11-bytes", tag(f["opt_i32"], 0) + b"\xff" * 10 + b"\x01")
    # Timestamp / Duration / Value / FieldMask range rules
    ts, du = f["ts"], f["dur"]
    sn = lambda s, n: (tag(1, 0) + vi(s) if s else b"") + (tag(2, 0) + vi(n) if n else b"")  # noqa: E731
    add("ts-nanos-max", ld(ts, sn(1, 999999999)))
    add("ts-min", ld(ts, sn(-62135596800, 0)))
    add("ts-max", ld(ts, sn(253402300799, 999999999)))
    add("ts-negative-seconds-nanos", ld(ts, sn(-1, 500000000)))
    add("ts-nanos-negative", ld(ts, sn(0, -1)))
    add("ts-nanos-1e9", ld(ts, sn(0, 1000000000)))
    add("ts-seconds-over", ld(ts, sn(253402300800, 0)))
    add("ts-seconds-under", ld(ts, sn(-62135596801, 0)))
    add("dur-max", ld(du, sn(315576000000, 999999999)))
    add("dur-min", ld(du, sn(-315576000000, -999999999)))
    add("dur-neg-nanos-only", ld(du, sn(0, -5)))
    add("dur-over", ld(du, sn(315576000001, 0)))
    add("dur-under", ld(du, sn(-315576000001, 0)))
    add("dur-sign-mismatch", ld(du, sn(1, -1)))
    add("dur-sign-mismatch-neg", ld(du, sn(-1, 1)))
    add("dur-nanos-over", ld(du, sn(0, 1000000000)))
    add("dur-list-sign-mismatch", ld(f["r_dur"], sn(1, 5)) + ld(f["r_dur"], sn(1, -1)))
    val = f["val"]
    add("value-number", ld(val, tag(2, 1) + struct.pack("<d", 2.5)))
    add("value-nan", ld(val, tag(2, 1) + struct.pack("<d", math.nan)))
    add("value-inf", ld(val, tag(2, 1) + struct.pack("<d", math.inf)))
    add("value-neg-inf-in-list",
        ld(f["lst"], ld(1, tag(2, 1) + struct.pack("<d", -math.inf))))
    add("value-nan-in-struct",
        ld(f["st"], ld(1, ld(1, b"k") + ld(2, tag(2, 1) + struct.pack("<d", math.nan)))))
    add("mask-snake", ld(f["mask"], ld(1, b"foo_bar.baz") + ld(1, b"q")))
    add("mask-camel-path", ld(f["mask"], ld(1, b"fooBar")))
    add("mask-double-underscore", ld(f["mask"], ld(1, b"foo__bar")))
    add("mask-trailing-underscore", ld(f["mask"], ld(1, b"foo_")))
    add("mask-underscore-digit", ld(f["mask"], ld(1, b"foo_1")))
    add("field-number-zero", tag(0, 0) + vi(1))
    add("field-number-zero-len", b"\x02\x01a")
    add("field-number-zero-after", tag(f["opt_i32"], 0) + vi(1) + tag(0, 0) + vi(1))
    return c


def _nonminimal_tag(field: int, wt: int) -> bytes:
    """Tag varint padded with one redundant continuation byte."""
    t = bytearray(tag(field, wt))
    t[-1] |= 0x80
    return bytes(t) + b"\x00"


ACCEPT = _accept_cases()
REJECT = _reject_cases()
WIRES = _wire_cases()

# The WIRES ids json_format refuses (malformed wire, or a value protojson
# will not print).  Pinned so that a protobuf upgrade or a typo in a case
# cannot quietly turn a value comparison into a mere status check:
# test_wires_oracle_verdicts_pinned compares the oracle against this set.
WIRES_ORACLE_REJECTS = frozenset("""
    string-invalid-utf8 trunc-len trunc-packed-fixed32 trunc-packed-double
    trunc-varint trunc-tag len-over-32-bits len-over-32-bits-packed
    len-wrap-unknown-2^64-k len-wrap-unknown-2^64-k-tail
    len-wrap-in-group-2^64-k len-wrap-mismatch-2^64-k len-wrap-string-2^64-k
    len-wrap-in-entry-2^64-k len-wrap-unknown-2^64-1
    len-wrap-unknown-2^64-1-tail len-wrap-in-group-2^64-1
    len-wrap-mismatch-2^64-1 len-wrap-string-2^64-1 len-wrap-in-entry-2^64-1
    len-wrap-unknown-2^32+small len-wrap-unknown-2^32+small-tail
    len-wrap-in-group-2^32+small len-wrap-mismatch-2^32+small
    len-wrap-string-2^32+small len-wrap-in-entry-2^32+small
    len-wrap-unknown-2^63 len-wrap-unknown-2^63-tail len-wrap-in-group-2^63
    len-wrap-mismatch-2^63 len-wrap-string-2^63 len-wrap-in-entry-2^63
    len-wrap-back-to-tag len-wrap-back-to-tag-in-group
    group-end-number-differs group-interleaved group-inner-end-differs
    end-group-alone group-unterminated trunc-nested trunc-fixed64
    varint-11-bytes ts-nanos-negative ts-nanos-1e9 ts-seconds-over
    ts-seconds-under dur-over dur-under dur-sign-mismatch
    dur-sign-mismatch-neg dur-nanos-over dur-list-sign-mismatch value-nan
    value-inf value-neg-inf-in-list value-nan-in-struct mask-camel-path
    mask-double-underscore mask-trailing-underscore mask-underscore-digit
    field-number-zero field-number-zero-len field-number-zero-after
""".split())

# at most one ACCEPT+WIRES case in eight may carry a HOST tag
HOST_CAP = 8


# ---- comparison rules ---------------------------------------------------------

_DOUBLE_WKT = {"google.protobuf.Struct", "google.protobuf.Value",
               "google.protobuf.ListValue"}
_STRING_WKT = {"google.protobuf.Timestamp", "google.protobuf.Duration",
               "google.protobuf.FieldMask"}
_NONFINITE = ("NaN", "Infinity", "-Infinity")


def _is_num(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _bits(x: float, kind: str) -> Optional[bytes]:
    """IEEE bytes at the field's precision; None for NaN (all NaNs equal)."""
    if math.isnan(x):
        return None
    if kind == "float":
        try:
            return struct.pack("<f", x)
        except OverflowError:
            return struct.pack("<f", math.copysign(math.inf, x))
    return struct.pack("<d", x)


def _fp_eq(a, b, kind: str) -> bool:
    """double: equal as Python floats; float: equal once both sides are
    packed to float32.  NaN equals NaN, -0.0 differs from 0.0."""
    for x in (a, b):
        if not (_is_num(x) or x in _NONFINITE):
            return False
    return _bits(float(a), kind) == _bits(float(b), kind)


def _exact(a, b) -> bool:
    return type(a) is type(b) and a == b


def _any_json_eq(a, b) -> bool:
    """Struct/Value/ListValue content: numbers are doubles."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_any_json_eq(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_any_json_eq(x, y) for x, y in zip(a, b))
    if _is_num(a) and _is_num(b):
        return _fp_eq(a, b, "double")
    return _exact(a, b)


def _field_eq(a, b, fd) -> bool:
    if fd.type == fd.TYPE_MESSAGE:
        return same_json(a, b, fd.message_type)
    if fd.type == fd.TYPE_FLOAT:
        return _fp_eq(a, b, "float")
    if fd.type == fd.TYPE_DOUBLE:
        return _fp_eq(a, b, "double")
    return _exact(a, b)


def same_json(a, b, desc) -> bool:
    """Compare two protojson values of message type ``desc`` (as produced by
    ``json.loads`` or ``MessageToDict``): structure, strings, ints and bools
    exactly; double/float fields by the precision rules above."""
    full = desc.full_name
    if full in _DOUBLE_WKT:
        return _any_json_eq(a, b)
    if full in _STRING_WKT:
        return _exact(a, b)
    if full.startswith("google.protobuf.") and full.endswith("Value"):
        return _field_eq(a, b, desc.fields_by_name["value"])
    if not (isinstance(a, dict) and isinstance(b, dict)) or a.keys() != b.keys():
        return False
    by_json = {fd.json_name: fd for fd in desc.fields}
    for k in a:
        fd = by_json.get(k)
        if fd is None:
            return False
        x, y = a[k], b[k]
        if fd.message_type is not None and fd.message_type.GetOptions().map_entry:
            vfd = fd.message_type.fields_by_name["value"]
            if not (isinstance(x, dict) and isinstance(y, dict)) or x.keys() != y.keys():
                return False
            if not all(_field_eq(x[m], y[m], vfd) for m in x):
                return False
        elif fd.is_repeated:
            if not (isinstance(x, list) and isinstance(y, list)) or len(x) != len(y):
                return False
            if not all(_field_eq(p, q, fd) for p, q in zip(x, y)):
                return False
        elif not _field_eq(x, y, fd):
            return False
    return True


def loads(text):
    """json.loads that keeps the sign of ``-0``: protojson prints negative
    zero as ``-0`` (an integer token to Python, which would drop the sign).
    In an integer field the resulting float then fails the exact compare."""
    return json.loads(text, parse_int=lambda t: -0.0 if t == "-0" else int(t))


def duplicate_members(text) -> List[str]:
    """Names that occur twice in one JSON object of ``text`` (json.loads
    silently keeps the last one)."""
    dups: List[str] = []

    def hook(pairs):
        seen = set()
        for k, _ in pairs:
            if k in seen:
                dups.append(k)
            seen.add(k)
        return dict(pairs)

    json.loads(text, object_pairs_hook=hook)
    return dups


# ---- oracle + batch runners ---------------------------------------------------

def oracle_parse(cls, text: str):
    """json_format on the real message class -> message, or None if it raises."""
    try:
        return json_format.Parse(text, cls())
    except json_format.ParseError:
        return None


def oracle_print(cls, wire: bytes) -> Optional[str]:
    """Wire -> protojson text, or None where the oracle refuses (malformed
    wire, or a value protojson will not print)."""
    try:
        msg = cls.FromString(wire)
        return json_format.MessageToJson(msg, indent=None, ensure_ascii=False)
    except (DecodeError, json_format.SerializeToJsonError):
        return None


def _verdict(case: Case, status: int, oracle_ok: bool, equal) -> Optional[str]:
    """The accept/reject contract.  ``equal`` is a thunk, evaluated only for
    a status-0 slot the oracle accepts.  Returns None or a failure text."""
    if not oracle_ok:
        return None if status != 0 else "oracle rejects, kernel returned status 0"
    if status == 0:
        return equal()
    if case.host and status in HOST_STATUSES:
        return None
    why = " (HOST-tagged: only 6/7 allowed)" if case.host else ""
    return f"oracle accepts, kernel status {status}{why}"


def run_encode(env: Env, cases: Sequence[Case]) -> dict:
    """One k_json2pb batch over ``cases``; case id -> None | failure text."""
    enc, pbs = env.engine.encode_batch(
        [c.data.encode() for c in cases], mode=1,
        msg_indices=[env.sink_idx] * len(cases), enforce=False)
    desc = env.sink_cls.DESCRIPTOR
    out = {}
    for c, r, pb in zip(cases, enc, pbs):
        want = oracle_parse(env.sink_cls, c.data)

        def equal(pb=pb, want=want):
            try:
                got = env.sink_cls.FromString(pb)
            except Exception as exc:
                return f"kernel wire does not parse: {exc!r} {pb!r}"
            g = json_format.MessageToDict(got)
            o = json_format.MessageToDict(want)
            if same_json(g, o, desc):
                return None
            return f"\nkernel: {g}\noracle: {o}"

        out[c.id] = _verdict(c, int(r["status"]), want is not None, equal)
        if out[c.id]:
            out[c.id] += f"  [aux={int(r['aux'])}] input={c.data[:200]!r}"
    return out


def _decode_verdicts(env, cases, wires, dec, outs, unwrap) -> dict:
    desc = env.sink_cls.DESCRIPTOR
    out = {}
    for c, w, r, o in zip(cases, wires, dec, outs):
        want = oracle_print(env.sink_cls, w)

        def equal(o=o, want=want):
            try:
                text = unwrap(o)
                g = loads(text)
            except Exception as exc:
                return f"kernel text is not JSON: {exc!r} {o!r}"
            if same_json(g, loads(want), desc):
                # docs/PARITY.md: wire with a repeated map key prints both
                # members (last one wins for any JSON reader, as compared
                # above); nothing else may print a name twice
                dups = [] if c.host == DUP_KEYS else duplicate_members(text)
                return f"duplicate JSON members {dups}: {o!r}" if dups else None
            return f"\nkernel: {o!r}\noracle: {want!r}"

        out[c.id] = _verdict(c, int(r["status"]), want is not None, equal)
        if out[c.id]:
            out[c.id] += f"  wire={w.hex()[:200]}"
    return out


def run_decode(env: Env, cases: Sequence[Case], wires: Sequence[bytes],
               mode: int = 1) -> dict:
    """One k_pb2json batch.  Mode 1 compares the bare JSON; mode 0 first
    primes the request ids with an envelope encode batch of the same size,
    then compares the text inside result.content[0].text — the second
    escaping pass over text full of quotes."""
    n = len(cases)
    idx = [env.sink_idx] * n
    if mode == 0:
        bodies = [json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/call",
                              "params": {"name": env.sink_tool,
                                         "arguments": {}}}).encode()
                  for i in range(n)]
        enc, _ = env.engine.encode_batch(bodies, mode=0)
        assert all(int(r["status"]) == 0 for r in enc)

        def unwrap(o):
            resp = json.loads(o)
            assert resp["result"]["isError"] is False
            return resp["result"]["content"][0]["text"]
    else:
        unwrap = lambda o: o  # noqa: E731
    dec, outs = env.engine.decode_batch(list(wires), idx, mode=mode)
    res = _decode_verdicts(env, cases, wires, dec, outs, unwrap)
    if mode == 0:
        for i, (c, o) in enumerate(zip(cases, outs)):
            if o is not None and res[c.id] is None and json.loads(o)["id"] != i:
                res[c.id] = f"envelope id {json.loads(o)['id']} in slot {i}"
    return res


def accept_wires(env: Env) -> List[bytes]:
    """The oracle's own serialization of every ACCEPT payload."""
    return [json_format.Parse(c.data, env.sink_cls()).SerializeToString()
            for c in ACCEPT]


# ---- lane-window sweep --------------------------------------------------------
#
# The CPU build runs the kernels at WAVE=1, where every ballot/shuffle/SWAR
# window is a serial loop; only gfx950 can judge the lane-parallel forms.
# These generators place the interesting byte at every window edge: the
# 64-byte skip_ws window, the 256-byte (4 bytes x 64 lanes) windows of
# string_end / utf8_span_valid / wave_copy / put_escaped, and the 192-byte
# put_base64 pass.  The oracles are json, Python's strict UTF-8 decoder,
# base64 and json_format — never the kernel itself.

MAX_BATCH = 4096

STRING_LENGTHS = (list(range(0, 71)) + list(range(120, 137))
                  + list(range(248, 265)) + list(range(504, 521))
                  + list(range(1016, 1033)))
SPECIALS = ['"', "\\", "\n", "\x01", "\x1f", "\x7f", "é", "中", "😀"]


def sweep_strings() -> List[str]:
    """'a'*L with one special character at 0, L//2 and each of the last
    five positions, for every window-edge length."""
    out = [""]
    for n in STRING_LENGTHS:
        if n == 0:
            continue
        for pos in sorted({0, n // 2} | {p for p in range(n - 5, n) if p >= 0}):
            for sp in SPECIALS:
                out.append("a" * pos + sp + "a" * (n - pos - 1))
    return out


def _chunks(seq, n):
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


def _encode_inner(env: Env, bodies: Sequence[bytes], filler: bytes):
    """k_json2pb over bench.Inner payloads, chunked to the engine's batch
    limit, each chunk led by ``filler`` so every slot start shifts with it.
    Returns [(status, wire|None)] without the fillers."""
    res = []
    for part in _chunks(list(bodies), MAX_BATCH - 1):
        batch = [filler] + part
        enc, pbs = env.engine.encode_batch(
            batch, mode=1, msg_indices=[env.inner_idx] * len(batch), enforce=False)
        assert int(enc[0]["status"]) == 0, "filler slot"
        res += [(int(r["status"]), pb) for r, pb in zip(enc[1:], pbs[1:])]
    return res


def _decode_inner(env: Env, wires: Sequence[Optional[bytes]], filler: bytes,
                  mode: int):
    res = []
    for part in _chunks(list(wires), MAX_BATCH - 1):
        batch = [filler] + part
        if mode == 0:
            bodies = [json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/call",
                                  "params": {"name": env.sink_tool,
                                             "arguments": {}}}).encode()
                      for i in range(len(batch))]
            enc, _ = env.engine.encode_batch(bodies, mode=0)
            assert all(int(r["status"]) == 0 for r in enc)
        dec, outs = env.engine.decode_batch(batch, [env.inner_idx] * len(batch),
                                            mode=mode)
        assert int(dec[0]["status"]) == 0, "filler slot"
        res += [(int(r["status"]), o) for r, o in zip(dec[1:], outs[1:])]
    return res


# leading filler slots: each one byte longer than the last, so the slots
# behind it (packed back to back) start at every residue mod 4
JSON_FILLERS = [b"{}" + b" " * k for k in range(4)]
WIRE_FILLERS = [ld(1, b"x" * k) for k in range(1, 5)]


def _first_diff(runs) -> Optional[str]:
    for k, run in enumerate(runs[1:], 1):
        for i, (a, b) in enumerate(zip(runs[0], run)):
            if a != b:
                return f"slot {i}: alignment run {k} differs from run 0: {a!r} vs {b!r}"
    return None


def check_string_sweep(env: Env) -> Optional[str]:
    """Every sweep string through encode (raw UTF-8 and \\uXXXX JSON) and
    decode (bare and enveloped), at all four slot alignments."""
    strs = sweep_strings()
    cls = env.inner_cls
    want_wire = [cls(key=t) for t in strs]
    for ascii_ in (False, True):
        bodies = [json.dumps({"key": t}, ensure_ascii=ascii_).encode() for t in strs]
        runs = [_encode_inner(env, bodies, fl) for fl in JSON_FILLERS]
        for t, (st, pb), want in zip(strs, runs[0], want_wire):
            if st != 0:
                return f"encode(ascii={ascii_}) status {st} for {t[:40]!r} len {len(t)}"
            try:
                got = cls.FromString(pb)
            except Exception as exc:
                return f"encode(ascii={ascii_}) wire unparsable ({exc!r}) len {len(t)}"
            if got != want:
                return (f"encode(ascii={ascii_}) len {len(t)}: kernel key "
                        f"{got.key[-12:]!r} != {t[-12:]!r}")
        bad = _first_diff(runs)
        if bad:
            return f"encode(ascii={ascii_}) {bad}"
    wires = [m.SerializeToString() for m in want_wire]
    for mode in (1, 0):
        runs = [_decode_inner(env, wires, fl, mode) for fl in WIRE_FILLERS]
        for i, (t, (st, o)) in enumerate(zip(strs, runs[0])):
            if st != 0:
                return f"decode(mode={mode}) status {st} for {t[:40]!r} len {len(t)}"
            try:
                g = json.loads(o)
                if mode == 0:
                    g = json.loads(g["result"]["content"][0]["text"])
            except Exception as exc:
                return f"decode(mode={mode}) not JSON ({exc!r}): {o[-60:]!r}"
            if g != ({"key": t} if t else {}):
                return f"decode(mode={mode}) len {len(t)}: {o[-60:]!r}"
        if mode == 1:
            # envelopes carry the slot's request id, which shifts with the
            # chunking; the bare texts must be byte-identical
            bad = _first_diff(runs)
            if bad:
                return f"decode(mode={mode}) {bad}"
        else:
            inner = [[(st, json.loads(o)["result"]["content"][0]["text"])
                      for st, o in run] for run in runs]
            bad = _first_diff(inner)
            if bad:
                return f"decode(mode={mode}) {bad}"
    return None


UTF8_DEFECTS = [b"\x80", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf5\x80\x80\x80"]
UTF8_OFFSETS = (list(range(0, 9)) + list(range(60, 69)) + list(range(250, 261))
                + list(range(296, 300)))
UTF8_VALID = ["é", "中", "😀"]


def utf8_cases() -> List[bytes]:
    """300-byte strings: one defect at every window-edge offset (plus a
    sequence truncated by the end of the string), mirrored by VALID 2/3/4-
    byte sequences whose lead byte sits on the last byte of a dword, of the
    64-byte window and of the 256-byte window."""
    out = []
    base = b"a" * 300
    for off in UTF8_OFFSETS:
        for d in UTF8_DEFECTS:
            if off + len(d) <= 300:
                out.append(base[:off] + d + base[off + len(d):])
    out.append(base[:298] + b"\xe2\x82")
    for lead in (3, 63, 255, 2, 62, 254, 4, 64, 256):
        for ch in UTF8_VALID:
            e = ch.encode()
            out.append(base[:lead] + e + base[lead + len(e):])
    return out


def check_utf8(env: Env) -> Optional[str]:
    cases = utf8_cases()
    runs_e, runs_d = [], []
    for jf, wf in zip(JSON_FILLERS, WIRE_FILLERS):
        enc = _encode_inner(env, [b'{"key":"' + b + b'"}' for b in cases], jf)
        dec = _decode_inner(env, [ld(1, b) for b in cases], wf, 1)
        runs_e.append(enc)
        runs_d.append(dec)
        for b, (es, pb), (ds, o) in zip(cases, enc, dec):
            try:
                text = b.decode("utf-8")  # strict: the oracle
            except UnicodeDecodeError:
                text = None
            where = f"bytes {b.strip(b'a')!r} at {len(b) - len(b.lstrip(b'a'))}"
            if text is None:
                if es != E_PARSE:
                    return f"invalid UTF-8 {where}: encode status {es}, want E_PARSE"
                if ds != E_UNSUPPORTED:
                    return f"invalid UTF-8 {where}: decode status {ds}, want E_UNSUPPORTED"
            else:
                if es != 0 or env.inner_cls.FromString(pb).key != text:
                    return f"valid UTF-8 {where}: encode status {es} or value differs"
                if ds != 0 or json.loads(o) != {"key": text}:
                    return f"valid UTF-8 {where}: decode status {ds} or value differs"
    return _first_diff(runs_e) or _first_diff(runs_d)


WS_RUNS = (list(range(0, 4)) + list(range(62, 67)) + list(range(126, 131))
           + list(range(254, 259)))


def whitespace_cases() -> List[bytes]:
    toks = ["{", '"key"', ":", '"v"', ",", '"value"', ":", '"7"', "}"]
    out = []
    for gap in range(len(toks) + 1):          # before '{' ... after '}'
        for n in WS_RUNS:
            ws = "".join(" \t\n\r"[(i + gap) % 4] for i in range(n))
            out.append(("".join(toks[:gap]) + ws + "".join(toks[gap:])).encode())
    return out


def check_whitespace(env: Env) -> Optional[str]:
    cases = whitespace_cases()
    want = env.inner_cls(key="v", value=7)
    for b in cases:
        assert json_format.Parse(b.decode(), env.inner_cls()) == want
    runs = [_encode_inner(env, cases, fl) for fl in JSON_FILLERS]
    for b, (st, pb) in zip(cases, runs[0]):
        n = len(b) - 23
        if st != 0:
            return f"{n} whitespace bytes in {b[:12]!r}...: status {st}"
        if env.inner_cls.FromString(pb) != want:
            return f"{n} whitespace bytes in {b[:12]!r}...: value differs"
    return _first_diff(runs)


B64_LENGTHS = list(range(0, 9)) + list(range(189, 196)) + list(range(381, 388))


def check_base64(env: Env) -> Optional[str]:
    """bytes <-> base64 across the 192-byte put_base64 pass boundary, input
    given in std, url-safe and unpadded forms."""
    datas = []
    for n in B64_LENGTHS:
        datas.append(bytes((i * 73 + 251) & 0xFF for i in range(n)))
        datas.append(b"\xff" * n)       # all '/' (or '_'): alphabet edge
        datas.append(b"\xfb\xef\xbe" * (n // 3) + b"\xfb" * (n % 3))  # '+' / '-'
    wires = [env.sink_cls(blob=d).SerializeToString() for d in datas]
    dec, outs = env.engine.decode_batch(wires, [env.sink_idx] * len(wires), mode=1)
    for d, r, o in zip(datas, dec, outs):
        if int(r["status"]) != 0:
            return f"decode {len(d)} bytes: status {int(r['status'])}"
        want = ({"blob": base64.b64encode(d).decode()} if d else {})
        if json.loads(o) != want:
            return f"decode {len(d)} bytes: {o[-40:]!r} != ...{want['blob'][-30:]!r}"
    forms = []
    for d in datas:
        std = base64.b64encode(d).decode()
        url = base64.urlsafe_b64encode(d).decode()
        for text in (std, url, std.rstrip("="), url.rstrip("=")):
            forms.append((d, text))
    enc, pbs = env.engine.encode_batch(
        [('{"blob":"%s"}' % t).encode() for _, t in forms], mode=1,
        msg_indices=[env.sink_idx] * len(forms), enforce=False)
    for (d, t), r, pb in zip(forms, enc, pbs):
        if int(r["status"]) != 0:
            return f"encode {len(d)} bytes as ...{t[-8:]!r}: status {int(r['status'])}"
        if env.sink_cls.FromString(pb).blob != d:
            return f"encode {len(d)} bytes as ...{t[-8:]!r}: value differs"
    return None


COMPACTION_SIZES = (1, 255, 256, 257, 513, 4096)


def check_compaction(env: Env, n: int) -> Optional[str]:
    """Decode n slots whose output lengths walk through every residue mod 4;
    every seventh slot is skipped (None) and every eleventh fails (invalid
    UTF-8), so zero and dead out_len values feed the offset scan.  A wrong
    offset shows as the neighbour's text (each slot's text is unique)."""
    wires: List[Optional[bytes]] = []
    want: List[Optional[dict]] = []
    for i in range(n):
        if i % 7 == 3:
            wires.append(None)
            want.append(None)
        elif i % 11 == 5:
            wires.append(ld(1, b"bad\x80"))
            want.append(None)
        else:
            m = env.inner_cls(key="k" * (i % 9), value=i + 1)
            wires.append(m.SerializeToString())
            want.append(json.loads(json_format.MessageToJson(m, indent=None)))
    dec, outs = env.engine.decode_batch(wires, [env.inner_idx] * n, mode=1)
    for i, (w, r, o) in enumerate(zip(want, dec, outs)):
        if w is None:
            if wires[i] is not None and int(r["status"]) != E_UNSUPPORTED:
                return f"n={n} slot {i}: invalid UTF-8 gave status {int(r['status'])}"
            continue
        if int(r["status"]) != 0:
            return f"n={n} slot {i}: status {int(r['status'])}"
        try:
            g = json.loads(o)
        except Exception:
            return f"n={n} slot {i}: not JSON: {o!r}"
        if g != w:
            return f"n={n} slot {i}: {o!r}, want {w}"
    return None


# ---- float32 text -----------------------------------------------------------

FLOAT_TIES = (1048576.25, 2097152.5, 0.15625)


def float32_values(seed: int, count: int = 8000) -> List[float]:
    """Random finite float32 bit patterns plus the tie-to-even values."""
    rng = random.Random(seed)
    vals = list(FLOAT_TIES)
    # subnormals carry fewer mantissa bits, so their shortest text is often
    # under six digits (8.9561e-41): 64 of them, plus both ends of the range
    for bits in [1, 0x007FFFFF, 63914] + [rng.getrandbits(23) | 1 for _ in range(61)]:
        vals.append(struct.unpack("<f", struct.pack("<I", bits))[0])
    vals.append(struct.unpack("<f", struct.pack("<I", 0x7F7FFFFF))[0])  # FLT_MAX
    drawn = 0
    while drawn < count:
        v = struct.unpack("<f", struct.pack("<I", rng.getrandbits(32)))[0]
        if math.isfinite(v):
            vals.append(v)
            drawn += 1
    return vals


def _sig_digits(text: str) -> int:
    m = text.lower().split("e")[0].replace(".", "").lstrip("-0")
    return len(m.rstrip("0")) or 1


def check_float32_format(env: Env, seed: int) -> Optional[str]:
    """decode: the text of a ``float`` field must parse back to the same
    float32 and use no more significant digits than numpy's unique repr."""
    import numpy as np

    vals = float32_values(seed)
    wires = [env.wide_cls(f08_float=v).SerializeToString() for v in vals]
    outs, dec = [], []
    for part in _chunks(wires, MAX_BATCH):
        d2, o2 = env.engine.decode_batch(part, [env.wide_idx] * len(part), mode=1)
        dec.extend(d2)
        outs.extend(o2)
    for v, r, o in zip(vals, dec, outs):
        # float32 values sit far inside the double range: no host escape
        if int(r["status"]) != 0:
            return f"{v!r}: status {int(r['status'])}"
        text = o.decode()
        got = loads(text).get("f08Float", 0.0)
        if struct.pack("<f", float(got)) != struct.pack("<f", v):
            return f"{v!r}: kernel text {text} parses to another float32"
        if v != 0.0:
            num = text.split(":", 1)[1].rstrip("}")
            ref = np.format_float_scientific(np.float32(v), unique=True)
            if _sig_digits(num) > _sig_digits(ref):
                return f"{v!r}: kernel text {num} is longer than {ref}"
    return None


def check_float32_parse(env: Env, seed: int) -> Optional[str]:
    """encode: JSON decimals of 1-12 digits must land on the float32 that
    struct.pack('<f', float(text)) gives (decimal -> double -> float32, both
    correctly rounded).  Go rounds decimal text to float32 in ONE step; the
    two can differ at exact double-rounding ties, which needs a decimal
    within half a double ulp of a float32 midpoint — out of scope here and
    out of reach of 12-digit inputs except at the ties themselves."""
    rng = random.Random(seed)
    texts = []
    for _ in range(8000):
        digs = "".join(rng.choices("0123456789", k=rng.randint(1, 12)))
        digs = rng.choice("123456789") + digs[1:]
        sign = "-" if rng.random() < 0.3 else ""
        texts.append(f"{sign}{digs[0]}.{digs[1:] or '0'}e{rng.randint(-30, 30)}")
    texts += [repr(v) for v in FLOAT_TIES] + ["16777217", "0.1", "1e-45", "3.4028234e38"]
    res = []
    for part in _chunks([('{"f08Float":%s}' % t).encode() for t in texts], MAX_BATCH):
        enc, pbs = env.engine.encode_batch(
            part, mode=1, msg_indices=[env.wide_idx] * len(part), enforce=False)
        res += list(zip(enc, pbs))
    for t, (r, pb) in zip(texts, res):
        if int(r["status"]) != 0:
            return f"{t}: status {int(r['status'])}"
        got = env.wide_cls.FromString(pb).f08_float
        if struct.pack("<f", got) != struct.pack("<f", float(t)):
            return f"{t}: kernel {got!r}, want {struct.unpack('<f', struct.pack('<f', float(t)))[0]!r}"
    return None
