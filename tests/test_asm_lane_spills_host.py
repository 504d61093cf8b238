"""tools/asm_lane_spills.py on a synthetic 30-line kernel with known counts in two nested loops (no GPU, no compiler)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import asm_lane_spills as als   # noqa: E402

# entry: 3 parks (one of vcc_lo) and a scratch store; outer loop BB0_1: 2 fetches, one designed read (lane in s7), one park,
# one scratch load, 3 other vector instructions; inner loop BB0_2: one fetch, one designed write (lane in m0), one write whose
# source is a constant (no spill), 2 other vector instructions; after the loops: one fetch.  A second kernel follows: not counted.
SNIPPET = """\t.text
_Z5probePf:                             ; @_Z5probePf
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\tv_writelane_b32 v40, s2, 0
\tv_writelane_b32 v40, s3, 1
\tv_writelane_b32 v40, vcc_lo, 2
\tscratch_store_dword off, v1, off offset:4 ; 4-byte Folded Spill
.LBB0_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_2 Depth 2
\tv_readlane_b32 s4, v40, 0
\tv_readlane_b32 s5, v40, 1
\tv_readlane_b32 s6, v41, s7
\tv_writelane_b32 v40, s8, 3
\tscratch_load_dword v2, off, off offset:4 ; 4-byte Folded Reload
\tv_add_u32_e32 v3, v2, v2
\tv_mov_b32_e32 v4, 0
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\tv_readlane_b32 s9, v40, 0x3
\tv_writelane_b32 v41, s9, m0
\tv_writelane_b32 v41, 0, 5
\tv_add_f32_e32 v5, v5, v3
\tv_mul_f32_e32 v5, v5, v5
\ts_cbranch_scc1 .LBB0_2
; %bb.3:                                ;   in Loop: Header=BB0_1 Depth=1
\tv_add_u32_e32 v4, 1, v4
\ts_cbranch_vccnz .LBB0_1
; %bb.4:
\tv_readlane_b32 s10, v40, 2
\ts_endpgm
.Lfunc_end0:
; TotalNumSgprs: 106
; NumVgprs: 96
; ScratchSize: 8
; Occupancy: 5
_Z5otherPf:                             ; @_Z5otherPf
; %bb.0:
\tv_readlane_b32 s4, v40, 0
\ts_endpgm
.Lfunc_end1:
; TotalNumSgprs: 8
; NumVgprs: 41
; ScratchSize: 0
; Occupancy: 8
"""


def counts(c):
    return tuple(c[k] for k in als.KEYS)   # rd, wr, var, scratch ld, scratch st, valu


def test_counts_per_loop_nest_of_a_synthetic_kernel():
    r = als.analyse(SNIPPET.split("\n"), "probe")
    assert r["order"] == ["BB0_1", "BB0_2"] and r["parents"] == {"BB0_1": [], "BB0_2": ["BB0_1"]}
    assert counts(r["own"][None]) == (1, 3, 0, 0, 1, 0)          # entry and exit
    assert counts(r["own"]["BB0_1"]) == (2, 1, 1, 1, 0, 3)       # outer loop without the inner one (%bb.3 is the outer loop's)
    assert counts(r["own"]["BB0_2"]) == (1, 0, 2, 0, 0, 2)
    assert counts(r["all"]["BB0_1"]) == (3, 1, 3, 1, 0, 5)       # ... with it
    assert counts(r["kernel"]) == (4, 4, 3, 1, 1, 5)
    assert r["meta"] == {"TotalNumSgprs": 106, "NumVgprs": 96, "ScratchSize": 8, "Occupancy": 5}


def test_the_second_kernel_is_found_by_name_and_a_missing_one_is_an_error():
    r = als.analyse(SNIPPET.split("\n"), "other")
    assert counts(r["kernel"]) == (1, 0, 0, 0, 0, 0) and r["meta"]["NumVgprs"] == 41 and r["order"] == []
    try:
        als.analyse(SNIPPET.split("\n"), "absent")
    except SystemExit as e:
        assert "absent" in str(e)
    else:
        raise AssertionError("no error for a kernel that is not there")


def test_the_command_line_prints_the_tables(tmp_path):
    p = tmp_path / "probe.s"
    p.write_text(SNIPPET)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_lane_spills.py"), str(p), "probe", "--lines"],
                         capture_output=True, text=True, check=True).stdout
    assert "whole kernel" in out and "rd    4  wr    4  var   3  scratch ld   1 st   1  valu     5" in out
    assert "loop BB0_2 depth 2" in out and "Sgpr 106  Vgpr 96  Scratch 8  Occupancy 5" in out
    assert "v_readlane_b32 s9, v40, 0x3" in out
