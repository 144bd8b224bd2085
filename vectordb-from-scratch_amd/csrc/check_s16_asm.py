#!/usr/bin/env python3
"""Build-time check of kernels_fused_s16.hip's generated code (called by the Makefile).

The kernel keeps its 256 accumulators in a[0:255] BY HAND (inline asm on fixed AccVGPRs); hipcc does not know that and would
use "free" AccVGPRs as spill space the moment register pressure rises -- silently overwriting accumulators.  So every
instance must come out of the compiler with
  * no scratch (a scratch reload is also a vector-memory operation that drains the DMA pipeline),
  * no AccVGPR access the compiler made up: every v_accvgpr_read/_write must be one of ours (the a[N] spelling of the asm
    strings; compiler-generated ones print as aN), and no v_accvgpr_mov,
  * exactly the MFMAs and accumulator reads the source spells out: nothing writes an accumulator but an MFMA, and a tile
    starts with the MFMAs whose C is the constant 0.
Usage: check_s16_asm.py kernels_fused_s16.s"""
import re
import sys

txt = open(sys.argv[1]).read()
bad = []
kernels = re.findall(r"^(_ZN3vdb16fused_s16_kernel\w+):", txt, flags=re.M)
if len(kernels) < 3:
    bad.append(f"expected 3 kernel instances, found {len(kernels)}")
for name in kernels:
    body = txt[txt.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    n_scratch = len(re.findall(r"^\s+scratch_", body, flags=re.M))
    made_up = re.findall(r"^\s+v_accvgpr_(?:write_b32 a\d|read_b32 v\d+, a\d|mov)", body, flags=re.M)
    ours_r = len(re.findall(r"^\s+v_accvgpr_read_b32 v\d+, a\[", body, flags=re.M))
    n_acc = len(re.findall(r"^\s+v_mfma_f32_32x32x16_bf16 a\[(\w+:\w+)\], v\[\d+:\d+\], v\[\d+:\d+\], a\[\1\]\s*$", body, flags=re.M))
    n_c0 = len(re.findall(r"^\s+v_mfma_f32_32x32x16_bf16 a\[\w+:\w+\], v\[\d+:\d+\], v\[\d+:\d+\], 0\s*$", body, flags=re.M))
    n_mfma = len(re.findall(r"^\s+v_mfma_", body, flags=re.M))
    sample = "ILb1E" in name                                           # fused_s16_kernel<SAMPLE = true, ..>
    if n_scratch:
        bad.append(f"{name}: {n_scratch} scratch instructions")
    if made_up:
        bad.append(f"{name}: {len(made_up)} compiler-generated AccVGPR accesses")
    # Accumulate forms (D = A B + D): 16 per k-step, two k-steps in each of the two half-stage bodies = 64; 96 in the diagnostics
    # build (its compute-only k-step 1).  C = 0 forms (D = A B + 0, how a tile starts: nothing zeroes an accumulator): the 16 of
    # the k-step 0 that opens a tile.  Every MFMA of the kernel is one of the two forms.  Accumulator reads: 256, twice in the
    # filter instances (the epilogue exists with and without the NaN test).
    want_r = 256 if sample else 512
    if ours_r != want_r:
        bad.append(f"{name}: {ours_r} accumulator reads ({want_r} expected)")
    if n_acc not in (64, 96) or n_c0 != 16 or n_mfma != n_acc + n_c0:
        bad.append(f"{name}: {n_acc} accumulate MFMAs (64 expected, 96 in the diagnostics build), {n_c0} with C = 0 (16 expected), {n_mfma} in all")
if bad:
    print("kernels_fused_s16: generated code violates the hand-allocated AccVGPR contract:\n  " + "\n  ".join(bad), file=sys.stderr)
    sys.exit(1)
print(f"kernels_fused_s16: {len(kernels)} instances, no scratch, no compiler-made AccVGPR access")
