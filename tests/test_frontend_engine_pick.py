"""A frontend worker takes a FREE span engine (frontend.cpp take_engine).

Two mock executors, two workers.  One request parks executor A inside
run_span (the mock's ``__hold__`` marker); round-robin alone would send every
second later span to A and leave it waiting behind the parked one while B
sits idle."""

import http.client
import json
import threading

from ggrmcp_amd.server.native_http import load_module


def _body(rid, args):
    return json.dumps({"jsonrpc": "2.0", "id": rid, "method": "tools/call",
                       "params": {"name": "t", "arguments": args}})


def _post(port, body, timeout):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=timeout)
    try:
        conn.request("POST", "/", body=body,
                     headers={"Content-Type": "application/json"})
        r = conn.getresponse()
        return r.status, json.loads(r.read())
    finally:
        conn.close()


def test_worker_skips_a_held_engine():
    mod = load_module()
    a, b = mod.MockSpanExecutor(), mod.MockSpanExecutor()
    fe = mod.Frontend("127.0.0.1", 0,
                      lambda bodies, sids, headers, verdicts=None: [],
                      lambda method, path, body, headers: (404, b"{}"),
                      batch_window_us=100, max_batch=4096, workers=2,
                      reactors=1)
    fe.set_native_span([a.span_handle(), b.span_handle()], [],
                       fallback_cb=lambda items: [])
    port = fe.start()
    held = {}

    def hold():
        held["resp"] = _post(port, _body(100, {"m": "__hold__"}), 15)

    t = threading.Thread(target=hold)
    t.start()
    try:
        assert a.wait_held(5.0), "the first span goes to engine 0"
        for rid in range(1, 5):
            status, resp = _post(port, _body(rid, {"a": rid}), 5)
            assert status == 200
            assert resp["result"]["content"][0]["text"].startswith("n=")
        assert (a.calls(), b.calls()) == (1, 4)
        assert "resp" not in held
        st = fe.native_stats()
        # every second span started its walk at the held engine
        assert st["engineFirstBusy"] >= 1
        assert st["engineWaitUs"] >= 0
    finally:
        a.release()
        t.join(15)
        fe.stop()
    assert not t.is_alive()
    status, resp = held["resp"]
    assert status == 200 and resp["result"]["isError"] is False
    assert (a.calls(), b.calls()) == (1, 4)
