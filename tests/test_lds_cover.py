"""tools/lds_cover.py on a short synthetic listing: a read covered by a counted
wait, reads drained by lgkmcnt(0), an open read, and the nop wait-state sum.
Prices: VALU 4, MFMA 8, s_nop n: n + 1, anything else 1."""
import importlib.util
import os

from conftest import REPO

_spec = importlib.util.spec_from_file_location("lds_cover", os.path.join(REPO, "tools", "lds_cover.py"))
lc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lc)

LISTING = """
	s_mov_b32 s0, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	ds_read_b64 v[0:1], v10                  ; at 0
	ds_read_b128 v[2:5], v11                 ; at 1
	v_add_u32_e32 v12, v0, v1                ; at 2 (not a use: the parser measures waits)
	v_mfma_i32_16x16x64_i8 v[20:23], v[2:5], v[6:9], 0   ; at 6
	s_nop 5                                  ; at 14
	s_waitcnt lgkmcnt(1)                     ; at 20: covers the b64 alone
	v_fma_f64 v[30:31], v[0:1], v[0:1], v[0:1]
	s_waitcnt vmcnt(0)                       ; no lgkmcnt: covers nothing
	s_nop 0
	s_waitcnt vmcnt(2) lgkmcnt(0)            ; at 27: drains the b128
	ds_read_b64 v[40:41], v10                ; at 28
	ds_write_b64 v13, v[30:31]               ; at 29: counts against lgkmcnt
	s_waitcnt lgkmcnt(1)                     ; at 30: the write may be out, the read is in
	ds_read_b128 v[44:47], v11               ; at 31: open
	v_mov_b32_e32 v1, v2
	s_cbranch_scc1 .LBB0_1
.LBB0_2:
	ds_read_b64 v[0:1], v10
	s_waitcnt lgkmcnt(0)
"""


def test_body_ends_at_the_next_label():
    body = lc.body_of(LISTING, ".LBB0_1")
    assert body[0].startswith("ds_read_b64") and body[-1].startswith("s_cbranch_scc1")
    assert len(body) == 16


def test_counted_wait_drain_and_open_read():
    res = lc.cover(LISTING, ".LBB0_1")
    r = res["reads"]
    assert [x["op"] for x in r] == ["ds_read_b64", "ds_read_b128", "ds_read_b64", "ds_read_b128"]
    # the counted wait covers the first read and leaves the second in flight
    assert (r[0]["at"], r[0]["dist"], r[0]["count"]) == (0, 20, 1)
    assert (r[0]["mfma_between"], r[0]["valu_between"]) == (1, 1)
    # lgkmcnt(0) drains the second: 1 + 4 + 8 + 6 + 1 + 4 + 1 + 1 = 26 cycles after its issue
    assert (r[1]["at"], r[1]["dist"], r[1]["count"]) == (1, 26, 0)
    # a write issued after the read counts: lgkmcnt(1) covers the read
    assert (r[2]["dist"], r[2]["count"]) == (2, 1)
    # no wait of the body covers the last read: open, distance to the body's end
    assert r[3]["count"] is None and r[3]["dist"] == 6
    assert res["lgkmcnt0"] == 1
    assert (res["mfma"], res["valu"], res["mfma_before_f64_fma"]) == (1, 3, 1)


def test_nop_wait_states():
    res = lc.cover(LISTING, ".LBB0_1")
    assert (res["nops"], res["nop_wait_states"]) == (2, 7)
    assert res["cycles"] == 37


def test_summary_by_width():
    s = lc.summary(lc.cover(LISTING, ".LBB0_1"))
    assert s["ds_read_b64"] == {"reads": 2, "open": 0, "near": 2, "near_drained": 0, "min": 2, "median": 11.0}
    assert s["ds_read_b128"]["open"] == 1 and s["ds_read_b128"]["near_drained"] == 1
