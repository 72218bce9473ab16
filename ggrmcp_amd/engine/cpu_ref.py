"""CPU golden transcoder — the differential-test oracle for the GPU kernels.

Uses google.protobuf.json_format (the canonical protojson implementation,
same semantics as the reference's protojson.Unmarshal/Marshal at
reflection.go:351-381).  Also serves as the explicit per-request fallback
for batch slots the kernels flag E_UNSUPPORTED (out-of-order wire fields,
oversized ids, the google.protobuf.Any shapes listed under "Host-escape
rules" in docs/KERNELS.md) — counted in engine stats, never silent.

Both directions pass the message's OWN descriptor pool: the gateway's
descriptors live in a private pool (descriptors/loader.py), and the type
URL of a google.protobuf.Any must resolve there, not in protobuf's
default pool.
"""

from __future__ import annotations

from typing import Optional

from google.protobuf import json_format, message_factory
from google.protobuf.descriptor import Descriptor


class CpuTranscoder:
    def __init__(self) -> None:
        self._cls_cache = {}

    def _cls(self, desc: Descriptor):
        cls = self._cls_cache.get(desc.full_name)
        if cls is None:
            cls = message_factory.GetMessageClass(desc)
            self._cls_cache[desc.full_name] = cls
        return cls

    def json_to_pb(self, desc: Descriptor, json_text: str) -> bytes:
        msg = json_format.Parse(
            json_text or "{}", self._cls(desc)(), descriptor_pool=desc.file.pool
        )
        return msg.SerializeToString()

    def pb_to_json(self, desc: Descriptor, wire: bytes,
                   unpopulated: bool = False) -> str:
        """``unpopulated`` also prints zero/empty fields without presence
        (protojson EmitUnpopulated; the decode kernel's DM_UNPOPULATED)."""
        msg = self._cls(desc).FromString(wire)
        return json_format.MessageToJson(
            msg, indent=None, ensure_ascii=False, preserving_proto_field_name=False,
            descriptor_pool=desc.file.pool,
            always_print_fields_with_no_presence=unpopulated,
        )

    def pb_to_message(self, desc: Descriptor, wire: bytes):
        return self._cls(desc).FromString(wire)
