"""The shapes that tests/test_caller_memory_gpu.py runs through the raw C ABI inside guard bands, one table per convolution
entry point.  tests/test_host_cpu.py walks the same tables to check the wrappers' workspace requests without a GPU."""
from collections import OrderedDict

RTOL = 2e-5            # tests/test_ops_gpu.py: exact-f32 MFMA paths against fp64

# (shape, act, stats, branch, tolerance of y; the existing test of that path)
FWD_CASES = OrderedDict([
    # split-K (64x64 tiles, 9 K ranges): test_splitk_handoff_equals_reduce_launch, 1e-5
    ("splitk_reduce_launch", ((4, 12, 16, 128, 128, 3, 3, 1, "SAME"), 1, False, "splitk", 1e-5)),
    ("splitk_handoff", ((4, 12, 16, 128, 128, 3, 3, 1, "SAME"), 1, False, "splitk+tickets", 1e-5)),
    # split-K + statistics (the small pass over y afterwards): test_conv2d_fwd_affine_stats_slice's path
    ("splitk_stats", ((4, 12, 16, 128, 128, 3, 3, 1, "SAME"), 0, True, "splitk+tickets", 1e-5)),
    # 8 K steps per tap... kiters = 2 < 8: never split, query 0 (test_conv2d_fwd CONV_CASES[3])
    ("unsplit_query0", ((2, 13, 10, 64, 32, 1, 1, 1, "SAME"), 1, True, "unsplit", RTOL)),
    # K = 12 <= 16: the 256x16 tile, split 6 ways (CONV_CASES[5])
    ("tile_256x16", ((2, 14, 19, 64, 12, 3, 4, 1, "VALID"), 1, False, "256x16", RTOL)),
    # the VAE heads' dense layer on the skinny kernels: test_skinny_dense_gradients, 2e-6
    ("skinny", ((32, 1, 1, 28416, 300, 1, 1, 1, "VALID"), 0, False, "skinny", 2e-6)),
    # few-channel MFMA (act NONE, >= 65536 pixels), one statistics row per workgroup: test_few_channel_mfma_conv_matches_fp64
    ("few_channel_mfma", ((3, 150, 160, 8, 8, 3, 3, 1, "SAME"), 0, True, "few16", 2e-6)),
    # the direct kernel (ReLU keeps it off the MFMA form) and its stride-2 form: test_few_channel_direct_conv
    ("direct_relu", ((2, 200, 180, 8, 8, 3, 3, 1, "SAME"), 1, True, "direct", RTOL)),
    ("direct_stride2", ((3, 224, 298, 8, 8, 3, 3, 2, "SAME"), 0, True, "direct", RTOL)),
])


# (shape, residual, mask, tickets, branch, tolerance; the existing test of that path)
DGRAD_CASES = OrderedDict([
    # stride-1 split-K, both combine forms: test_splitk_handoff_equals_reduce_launch / test_conv2d_dgrad_wgrad
    ("s1_splitk_reduce_launch", ((4, 12, 16, 128, 128, 3, 3, 1, "SAME"), True, True, False, RTOL)),
    ("s1_splitk_handoff", ((4, 12, 16, 128, 128, 3, 3, 1, "SAME"), True, True, True, RTOL)),
    # stride == R == S, no padding: patch scatter (query 0 at this size)
    ("patch_scatter", ((2, 36, 48, 16, 32, 3, 3, 3, "SAME"), True, True, True, RTOL)),
    # stride 2, >= 16 channels written: the sub-pixel form (combined weights + its own split-K slabs)
    ("subpixel_3x3_same", ((1, 16, 20, 64, 64, 3, 3, 2, "SAME"), True, True, True, RTOL)),
    ("subpixel_2x3_valid", ((2, 12, 15, 32, 32, 2, 3, 2, "VALID"), True, True, False, RTOL)),
    # stride 2, 8 channels written: zero-inserted copy of gy in the workspace, then the stride-1 form behind it
    ("dilated_3x3_same", ((2, 17, 23, 8, 8, 3, 3, 2, "SAME"), True, True, True, RTOL)),
    ("dilated_3x2_valid", ((2, 15, 18, 8, 16, 3, 2, 2, "VALID"), True, True, False, RTOL)),
    # >= 65536 pixels: the few-channel MFMA form reads the zero-inserted view itself (no mask): test_few_channel_direct_conv, 3e-5
    ("few_channel_stride2", ((3, 224, 298, 8, 8, 3, 3, 2, "SAME"), True, False, False, 3e-5)),
    # ... and its stride-1 form on gy itself (the shape of FWD_CASES / WGRAD_CASES "few_channel_*"; 3e-5 as above)
    ("few_channel_stride1", ((3, 150, 160, 8, 8, 3, 3, 1, "SAME"), True, False, False, 3e-5)),
    # ... and with a ReLU mask neither MFMA nor direct form applies: dilated copy, then the implicit GEMM (exact f32)
    ("dilated_then_igemm_65536", ((3, 224, 298, 8, 8, 3, 3, 2, "SAME"), True, True, True, 3e-5)),
    # 112x149 8 -> 32: the 16-row instance of the halo kernel (test_few_channel_mfma_conv_matches_fp64 (3,147,161,8,32), 3e-5)
    ("halo16_narrow", ((4, 112, 149, 8, 32, 3, 3, 1, "SAME"), True, True, False, 3e-5)),
    # not 3x3, <= 16 gy channels, >= 65536 pixels, no mask: the direct kernel (3e-5 as its stride-2 cases)
    ("direct", ((2, 200, 190, 8, 16, 2, 3, 1, "VALID"), True, False, False, 3e-5)),
    ("skinny", ((32, 1, 1, 28416, 300, 1, 1, 1, "VALID"), True, True, False, 2e-6)),
])


# (shape, entry, tolerance; the existing test of that path)
WGRAD_CASES = OrderedDict([
    # 128 columns: 128-column tiles, 18 slabs (test_conv2d_dgrad_wgrad (2,18,24,256,128), RTOL; split3: 3e-5 as
    # test_wgrad_split3_geometries)
    ("cols128_f32", ((2, 18, 24, 256, 128, 3, 3, 1, "SAME"), "f32", RTOL)),
    ("cols128_split3", ((2, 18, 24, 256, 128, 3, 3, 1, "SAME"), "split3", 3e-5)),
    # 133 (padded 136) and 144 columns: 64-column tiles
    ("cols133_f32", ((8, 12, 16, 128, 133, 3, 3, 1, "SAME"), "f32", RTOL)),
    ("cols144_f32", ((8, 12, 16, 128, 144, 3, 3, 1, "SAME"), "f32", RTOL)),
    ("cols144_split3", ((8, 12, 16, 128, 144, 3, 3, 1, "SAME"), "split3", 3e-5)),
    # few channels through the fp32 entry onto the halo-16 kernel, 512 slabs: test_few_channel_wgrad_on_the_halo16_kernel, 2e-5
    ("few_channel_halo", ((3, 150, 160, 8, 8, 3, 3, 1, "SAME"), "f32", 2e-5)),
    # 32 -> 32 at 112x149 on the halo-16 kernel, 256 slabs ("one slab per CU"): test_wgrad_halo16_matches_fp64, 4e-5 / 2e-5
    ("halo16_split3", ((4, 112, 149, 32, 32, 3, 3, 1, "SAME"), "split3", 4e-5)),
    ("halo16_bf16", ((4, 112, 149, 32, 32, 3, 3, 1, "SAME"), "bf16", 2e-5)),
    # ... with the producer's batch norm applied on load: test_batch_norm_affine_applied_while_staging, 2e-5 against the same
    # entry on the materialised tensor
    ("halo16_affine_split3", ((4, 112, 149, 32, 32, 3, 3, 1, "SAME"), "affine1", 2e-5)),
    ("few_channel_affine", ((3, 150, 160, 8, 8, 3, 3, 1, "SAME"), "affine0", 2e-5)),
    ("skinny", ((32, 1, 1, 28416, 300, 1, 1, 1, "VALID"), "f32", 2e-6)),
    # 128 pixels: one slab, so the split-MFMA kernels write dW and db themselves, no reduce (3e-5 as the split cases above) -
    # the per-tap kernel (16-pixel rows) and the tap-sharing kernel (32-pixel rows).  A db off a 16-byte boundary cannot take
    # their 16-byte row stores: tests/test_operand_forms_gpu.py
    ("unsplit_split3", ((1, 8, 16, 64, 64, 3, 3, 1, "SAME"), "split3", 3e-5)),
    ("unsplit_tap", ((1, 4, 32, 64, 64, 3, 3, 1, "SAME"), "split3", 3e-5)),
])


# (shape, tolerances fwd / dgrad / wgrad; test_deconv: RTOL, test_deconv_dgrad_few_channels_direct: 2e-6 / 3e-5 / 2e-5)
DECONV_CASES = OrderedDict([
    ("scatter_gap_fill", ((2, 12, 16, 128, 128, 2, 2, 3), RTOL, RTOL, RTOL)),       # kernel < stride: gaps receive the bias
    ("subpixel", ((2, 7, 9, 64, 32, 2, 3, 2), RTOL, RTOL, RTOL)),                   # kernel > stride, >= 16 outputs
    ("dilated", ((2, 6, 8, 32, 8, 3, 3, 2), RTOL, RTOL, RTOL)),                     # kernel > stride, 8 outputs: zero-inserted x
    ("pointwise_patch2", ((5, 112, 149, 32, 8, 2, 2, 2), 2e-6, 3e-5, 2e-5)),        # patch2_32x8 kernels, one slab per workgroup
    ("direct_dgrad", ((2, 190, 180, 8, 8, 2, 2, 2), RTOL, 3e-5, RTOL)),             # <= 16 gy channels, >= 65536 pixels, no mask
])
