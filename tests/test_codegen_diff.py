"""tools/codegen_diff.py on three short synthetic listings (no hipcc): a listing is identical to itself, a copy with two registers renamed and a
scratch offset moved is the same code, a copy with one instruction added differs."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import codegen_diff  # noqa: E402

LISTING = """\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.text
\t.p2align\t2
\t.type\t_Z6helperPm,@function
_Z6helperPm:                            ; @_Z6helperPm
; %bb.0:
\ts_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)
\tv_mov_b32_e32 v2, v0
\tscratch_store_dword off, v2, off offset:16
\ts_setpc_b64 s[30:31]
.Lfunc_end0:
\t.size\t_Z6helperPm, .Lfunc_end0-_Z6helperPm
\t.globl\t_Z1kPm
\t.p2align\t8
\t.type\t_Z1kPm,@function
_Z1kPm:                                 ; @_Z1kPm
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\tv_lshlrev_b32_e32 v1, 3, v0
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dwordx2 v[2:3], v1, s[2:3]
\ts_waitcnt vmcnt(0)
\tv_add_u32_e32 v2, 1, v2
\tglobal_store_dwordx2 v1, v[2:3], s[2:3]
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z1kPm
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 32
\t\t.amdhsa_next_free_vgpr 4
\t\t.amdhsa_next_free_sgpr 4
\t.end_amdhsa_kernel
\t.text
.Lfunc_end1:
\t.size\t_Z1kPm, .Lfunc_end1-_Z1kPm
\t.type\t__hip_cuid_0123456789abcdef,@object
\t.globl\t__hip_cuid_0123456789abcdef
__hip_cuid_0123456789abcdef:
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 0
    .name:           _Z1kPm
    .private_segment_fixed_size: 32
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         _Z1kPm.kd
    .vgpr_count:     4
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""
# the kernel's v1 and v[2:3] renamed, the helper's scratch slot moved, another compilation unit id
_HEAD, _KERNEL = LISTING.split("_Z1kPm:")
RENAMED = (_HEAD.replace("offset:16", "offset:24") + "_Z1kPm:"
           + _KERNEL.replace("v1,", "v5,").replace("v[2:3]", "v[6:7]").replace("v2", "v6").replace("0123456789abcdef", "fedcba9876543210"))
ADDED = LISTING.replace("\tv_add_u32_e32 v2, 1, v2\n", "\tv_add_u32_e32 v2, 1, v2\n\ts_nop 0\n")


def test_three_verdicts():
    assert codegen_diff.compare_listings(LISTING, LISTING) == {"_Z6helperPm": "identical", "_Z1kPm": "identical"}
    assert codegen_diff.compare_listings(LISTING, LISTING.replace("0123456789abcdef", "fedcba9876543210")) == {"_Z6helperPm": "identical", "_Z1kPm": "identical"}
    assert RENAMED != LISTING and codegen_diff.compare_listings(LISTING, RENAMED) == {"_Z6helperPm": "same code", "_Z1kPm": "same code"}
    assert codegen_diff.compare_listings(LISTING, ADDED) == {"_Z6helperPm": "identical", "_Z1kPm": "differs"}
    # the descriptor counts: a kernel whose instructions are the parent's but whose scratch grew is not the same code
    grown = LISTING.replace("private_segment_fixed_size 32", "private_segment_fixed_size 48").replace("private_segment_fixed_size: 32", "private_segment_fixed_size: 48").replace("offset:16", "offset:40")
    assert codegen_diff.compare_listings(LISTING, grown) == {"_Z6helperPm": "same code", "_Z1kPm": "differs"}
    assert codegen_diff.compare_listings(LISTING, LISTING.replace(".sgpr_count:     10", ".sgpr_count:     12"))["_Z1kPm"] == "differs"
