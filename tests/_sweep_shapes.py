"""Conv launch shapes of the geometry / batch sweep (tests/test_gpu_geometry_sweep.py) -- importable without the library so that
the host-only coverage test (tests/test_host_cpu.py) can hold the list against the launch-path variants and edge flags of
the whole domain.  The list is printed by tools/sweep_shapes.py; what counts is this file and the host test."""

#: (T, F) of the features: the benchmark's, 13 MFCCs, BirdCLEF-shaped patches, the net tests' sizes, short clips
SWEEP_FEATURE_SIZES = [(101, 40), (101, 13), (128, 128), (41, 20), (21, 12), (11, 40), (26, 40)]
#: forward launches: every train batch (a partial last one is any of 1..63) and the inference batches; backward: train only
SWEEP_FWD_BATCHES = tuple(range(1, 65)) + (100, 255, 256)
SWEEP_BWD_BATCHES = tuple(range(1, 65))


def integer_regime_is_exact(B, H, W, Cin, Cout, KS, stride):
    """x in {0..3}, w and dy in {-2..2}, bias in {-4..4}: every partial sum of the forward (|.| <= Cin*KS*KS*6 + 4), of the dgrad
    (<= Cout*KS*KS*4) and of the weight / bias gradient (<= M*6) is an integer below 2^24, hence exact in fp32 in ANY
    summation order."""
    M = B * (-(-H // stride)) * (-(-W // stride))
    return Cin * KS * KS * 6 + 4 < 2 ** 24 and Cout * KS * KS * 4 < 2 ** 24 and M * 6 < 2 ** 24


# B, H, W, Cin, Cout, KS, stride -- 105 cases, 1.1e+11 multiply-adds; behind each case the
# (variant: flags) pairs it was picked for (it exercises more)
SWEEP_CONVS = [
    (1, 51, 7, 16, 32, 1, 2),          # fwd<64,16,32,4,0>+tab: any odd_width one_image ragged; fwd<64,32,16,4,0>+stats+tab: any odd_width one_image  ...
    (1, 2, 5, 64, 128, 3, 1),          # fwd<128,128,32,2,0>+sk+tab: any odd_width one_image ragged window_exceeds_image; fwd<128,64,32,4,0>+sk+tab:  ...
    (1, 6, 3, 32, 64, 1, 2),           # fwd<64,32,32,4,0>+tab: any odd_width one_image ragged; fwd<64,64,32,2,0>+stats+tab: odd_width one_image ragg ...
    (1, 11, 5, 32, 64, 1, 2),          # fwd<64,32,32,4,0>+tab: odd_width one_image ragged; fwd<64,64,32,2,0>+stats+tab: odd_width one_image ragged;  ...
    (1, 6, 3, 64, 128, 5, 1),          # fwd<128,128,32,2,0>+sk+tab: odd_width one_image ragged window_exceeds_image; fwd<128,64,32,4,0>+sk+tab: odd_ ...
    (1, 101, 13, 16, 16, 3, 1),        # fwd<64,16,16,4,0>+stats+tab: any odd_width one_image ragged; fwd<64,16,16,4,0>+tab: any odd_width one_image  ...
    (1, 11, 6, 16, 32, 1, 2),          # fwd<64,16,32,4,0>+tab: one_image ragged; fwd<64,32,16,4,0>+stats+tab: one_image ragged; fwd<64,32,16,4,0>+ta ...
    (29, 6, 3, 32, 64, 5, 1),          # fwd<128,32,32,4,1>+sk+tab: any multi_image_tile odd_width ragged window_exceeds_image; fwd<128,64,32,4,0>+sk ...
    (1, 51, 7, 16, 32, 3, 1),          # fwd<128,16,32,4,0>+sk+tab: any odd_width one_image ragged; fwd<128,32,16,4,0>+sk+tab: any odd_width one_imag ...
    (1, 41, 20, 16, 16, 3, 1),         # fwd<64,16,16,4,0>+stats+tab: any one_image ragged; fwd<64,16,16,4,0>+tab: any one_image ragged; wgrad<16,64, ...
    (1, 101, 13, 32, 32, 3, 1),        # fwd<64,32,32,4,0>+stats+tab: any odd_width one_image ragged; wgrad<32,64,64>+tab+slabs: odd_width one_image  ...
    (1, 51, 20, 16, 32, 5, 1),         # fwd<128,16,32,4,0>+sk+tab: any one_image ragged; fwd<128,32,16,4,0>+sk+tab: one_image ragged; wgrad<32,64,64 ...
    (18, 3, 10, 32, 64, 5, 1),         # fwd<128,32,32,4,1>+sk+tab: multi_image_tile ragged window_exceeds_image; fwd<128,64,32,4,0>+sk+tab: multi_im ...
    (1, 21, 12, 16, 16, 3, 1),         # fwd<128,16,16,4,0>+sk+tab: any one_image ragged; wgrad<16,64,64>+tab: any one_image ragged
    (1, 11, 40, 16, 16, 3, 1),         # fwd<128,16,16,4,0>+sk+tab: any one_image ragged; wgrad<16,64,64>+tab: any one_image ragged
    (38, 101, 13, 16, 16, 3, 1),       # halo_fwd<3,256,16,4,false>: odd_width ragged tight_halo; halo_fwd<3,256,16,4,false>+stats: any odd_width rag ...
    (52, 2, 5, 64, 128, 3, 1),         # fwd<128,128,32,2,0>+sk+tab: multi_image_tile; wgrad<128,64,32>+tab+slabs: multi_image_tile odd_width ragged  ...
    (3, 6, 3, 32, 64, 1, 2),           # fwd<64,32,32,4,0>+tab: multi_image_tile; fwd<64,64,32,2,0>+stats+tab: multi_image_tile; fwd<64,64,32,2,0>+ta ...
    (3, 3, 10, 32, 64, 1, 2),          # fwd<64,32,32,4,0>+tab: multi_image_tile; fwd<64,64,32,2,0>+stats+tab: multi_image_tile; fwd<64,64,32,2,0>+ta ...
    (1, 6, 20, 32, 64, 3, 1),          # fwd<128,32,32,4,1>+sk+tab: one_image; halo_wgrad<3,5>: any one_image ragged
    (1, 13, 20, 32, 64, 3, 1),         # fwd<128,32,32,4,1>+sk+tab: one_image; halo_wgrad<3,5>: any one_image ragged
    (20, 13, 2, 64, 128, 3, 1),        # fwd<128,128,32,2,0>+sk+tab: multi_image_tile; wgrad<128,64,32>+tab+slabs: multi_image_tile ragged window_exc ...
    (1, 6, 20, 32, 64, 5, 1),          # halo_wgrad<5,5>: any one_image ragged
    (2, 51, 7, 32, 32, 3, 1),          # fwd<64,32,32,4,0>+stats+tab: odd_width ragged; wgrad<32,64,64>+tab+slabs: odd_width
    (3, 6, 20, 32, 64, 3, 1),          # halo_wgrad<3,5>+slabs: any multi_image_tile ragged
    (1, 13, 20, 32, 64, 5, 1),         # halo_wgrad<5,5>: any one_image ragged
    (49, 51, 20, 16, 32, 3, 1),        # halo_fwd<3,256,16,4,false>: ragged tight_halo; halo_fwd<3,256,32,4,false>: ragged tight_halo; halo_fwd<3,256 ...
    (1, 11, 40, 64, 64, 3, 1),         # halo_wgrad<3,10>: any one_image ragged
    (3, 6, 20, 32, 64, 5, 1),          # halo_wgrad<5,5>+slabs: any multi_image_tile ragged
    (38, 101, 13, 16, 16, 5, 1),       # halo_fwd<5,256,16,4,false>: odd_width ragged tight_halo; halo_fwd<5,256,16,4,false>+stats: any odd_width rag ...
    (1, 26, 40, 64, 64, 3, 1),         # halo_wgrad<3,10>+slabs: any one_image ragged
    (1, 11, 40, 64, 64, 5, 1),         # halo_wgrad<5,10>: any one_image ragged
    (1, 26, 40, 64, 64, 5, 1),         # halo_wgrad<5,10>+slabs: any one_image ragged
    (255, 51, 7, 16, 32, 3, 1),        # halo_fwd<3,256,32,4,false>: odd_width ragged tight_halo; halo_fwd<3,256,32,4,false>+stats: odd_width ragged  ...
    (255, 51, 7, 64, 128, 1, 2),       # fwd<128,64,32,4,0>+stats+tab: odd_width ragged; fwd<128,64,32,4,0>+tab: odd_width ragged
    (10, 11, 5, 32, 64, 3, 1),         # fwd<128,32,32,4,1>+sk+tab: odd_width; wgrad<64,64,64>+tab+slabs: odd_width
    (1, 51, 20, 32, 64, 3, 1),         # halo_wgrad<3,5>+slabs: one_image ragged
    (48, 64, 64, 16, 32, 1, 2),        # fwd<128,32,16,4,0>+stats+tab: any; fwd<128,32,16,4,0>+tab: any
    (255, 51, 20, 16, 32, 1, 2),       # fwd<128,32,16,4,0>+stats+tab: ragged; fwd<128,32,16,4,0>+tab: ragged
    (1, 51, 20, 32, 64, 5, 1),         # halo_wgrad<5,5>+slabs: one_image ragged
    (60, 41, 20, 16, 16, 5, 1),        # halo_fwd<5,256,16,4,false>: ragged tight_halo; halo_fwd<5,256,16,4,false>+stats: ragged tight_halo
    (3, 128, 128, 16, 16, 3, 1),       # fwd<128,16,16,4,0>+stats+tab: any; fwd<128,16,16,4,0>+tab: any
    (60, 41, 20, 16, 16, 3, 1),        # halo_fwd<3,256,16,4,false>+stats: ragged tight_halo
    (38, 101, 13, 32, 32, 5, 1),       # halo_fwd<5,256,32,4,false>: odd_width ragged tight_halo; halo_fwd<5,256,32,4,false>+stats: odd_width ragged  ...
    (255, 51, 20, 32, 64, 1, 2),       # fwd<128,64,32,4,0>+stats+tab: ragged; fwd<128,64,32,4,0>+tab: ragged
    (1, 101, 40, 64, 64, 3, 1),        # halo_wgrad<3,10>+slabs: one_image ragged
    (39, 2, 5, 512, 512, 3, 1),        # halo_fwd<3,128,64,2,true>+bal: multi_image_tile odd_width ragged tight_halo window_exceeds_image; wgrad<128, ...
    (3, 11, 6, 16, 32, 1, 2),          # wgrad<32,64,64>+tab: multi_image_tile
    (3, 6, 20, 16, 32, 1, 2),          # wgrad<32,64,64>+tab: multi_image_tile
    (3, 3, 2, 64, 128, 1, 2),          # wgrad<128,64,32>+tab: multi_image_tile
    (29, 11, 6, 16, 32, 1, 2),         # wgrad<32,64,64>+tab+slabs: multi_image_tile
    (18, 6, 20, 16, 32, 1, 2),         # wgrad<32,64,64>+tab+slabs: multi_image_tile
    (1, 6, 3, 32, 64, 5, 1),           # wgrad<64,64,64>+tab: window_exceeds_image
    (1, 3, 10, 32, 64, 5, 1),          # wgrad<64,64,64>+tab: window_exceeds_image
    (1, 64, 64, 32, 64, 1, 2),         # wgrad<64,64,64>+tab+slabs: one_image
    (5, 51, 7, 64, 128, 1, 2),         # wgrad<128,64,32>+tab+slabs: odd_width
    (1, 41, 20, 32, 32, 3, 1),         # fwd<64,32,32,4,0>+stats+tab: one_image
    (1, 64, 64, 64, 128, 1, 2),        # wgrad<128,64,32>+tab+slabs: one_image
    (1, 101, 13, 16, 16, 5, 1),        # fwd<128,16,16,4,0>+sk+tab: odd_width
    (49, 51, 20, 16, 32, 5, 1),        # halo_fwd<5,256,32,4,false>: ragged tight_halo; halo_fwd<5,256,32,4,false>+stats: ragged tight_halo
    (59, 51, 7, 32, 64, 5, 1),         # fwd<128,32,32,4,1>+bal+tab: any odd_width ragged; fwd<128,64,32,4,0>+bal+tab: any odd_width ragged
    (1, 32, 32, 32, 64, 3, 1),         # wgrad<64,64,64>+tab+slabs: one_image
    (1, 41, 20, 64, 64, 3, 1),         # halo_wgrad<3,5>+slabs: one_image
    (40, 101, 13, 64, 64, 3, 1),       # halo_fwd<3,128,64,2,false>: odd_width ragged tight_halo; halo_fwd<3,128,64,2,false>+stats: odd_width ragged  ...
    (1, 32, 32, 64, 128, 3, 1),        # wgrad<128,64,32>+tab+slabs: one_image
    (49, 51, 20, 32, 64, 3, 1),        # halo_fwd<3,128,64,2,false>: ragged tight_halo; halo_fwd<3,128,64,2,false>+stats: ragged tight_halo
    (1, 41, 20, 64, 64, 5, 1),         # halo_wgrad<5,5>+slabs: one_image
    (2, 11, 40, 64, 64, 5, 1),         # halo_wgrad<5,10>+slabs: ragged
    (48, 64, 64, 32, 64, 1, 2),        # fwd<128,32,32,4,1>+tab: any
    (48, 64, 64, 64, 128, 1, 2),       # fwd<128,128,32,2,0>+stats+tab: any; fwd<128,128,32,2,0>+tab: any
    (38, 101, 13, 32, 32, 3, 1),       # halo_fwd<3,256,32,4,false>: odd_width; halo_fwd<3,256,32,4,false>+stats: odd_width
    (35, 11, 5, 256, 256, 3, 1),       # halo_fwd<3,128,64,2,true>+bal: multi_image_tile odd_width ragged tight_halo
    (255, 51, 7, 16, 32, 5, 1),        # fwd<128,32,16,4,0>+stats+tab: odd_width ragged; fwd<128,32,16,4,0>+tab: odd_width ragged
    (255, 64, 64, 32, 64, 1, 2),       # fwd<128,64,16,4,0>+stats+tab: any; fwd<128,64,16,4,0>+tab: any
    (255, 51, 20, 64, 128, 1, 2),      # fwd<128,128,32,2,0>+stats+tab: ragged; fwd<128,128,32,2,0>+tab: ragged
    (13, 4, 5, 512, 512, 5, 1),        # fwd<128,128,32,2,0>+bal+tab: any multi_image_tile odd_width ragged window_exceeds_image
    (26, 2, 5, 512, 512, 5, 1),        # fwd<128,128,32,2,0>+bal+tab: any multi_image_tile odd_width ragged window_exceeds_image
    (24, 101, 13, 32, 32, 5, 1),       # fwd<128,32,32,4,1>+bal+tab: odd_width ragged
    (255, 51, 7, 32, 32, 5, 1),        # fwd<128,32,32,4,1>+stats+tab: any odd_width ragged; fwd<128,32,32,4,1>+tab: odd_width ragged
    (255, 11, 5, 64, 64, 5, 1),        # fwd<128,64,32,4,0>+bal+tab: multi_image_tile odd_width ragged
    (43, 6, 3, 512, 512, 5, 1),        # halo_fwd<5,128,64,2,true>+bal: multi_image_tile odd_width ragged window_exceeds_image; wgrad<128,128,32>+tab ...
    (31, 51, 20, 16, 32, 5, 1),        # fwd<128,16,32,4,0>+bal+tab: ragged
    (1, 101, 40, 64, 64, 5, 1),        # halo_wgrad<5,10>+slabs: one_image
    (8, 64, 64, 16, 32, 5, 1),         # fwd<128,16,32,4,0>+bal+tab: any
    (3, 128, 128, 32, 32, 3, 1),       # fwd<128,32,32,4,1>+stats+tab: any
    (49, 51, 20, 32, 64, 5, 1),        # halo_fwd<5,128,64,2,false>: ragged tight_halo; halo_fwd<5,128,64,2,false>+stats: ragged tight_halo
    (255, 21, 10, 32, 64, 5, 1),       # halo_fwd<5,128,64,2,false>: ragged tight_halo; halo_fwd<5,128,64,2,false>+stats: ragged tight_halo
    (12, 13, 5, 512, 512, 5, 1),       # halo_fwd<5,128,64,2,true>+bal: odd_width ragged tight_halo; wgrad<128,128,32>+tab: any multi_image_tile odd_ ...
    (57, 51, 7, 64, 64, 5, 1),         # wgrad<64,128,64>+tab+slabs: any odd_width ragged
    (255, 51, 7, 32, 64, 3, 1),        # halo_fwd<3,128,64,2,false>: odd_width; halo_fwd<3,128,64,2,false>+stats: odd_width
    (15, 13, 2, 512, 512, 3, 1),       # halo_fwd<3,128,64,2,true>+bal: window_exceeds_image
    (52, 26, 4, 128, 256, 5, 1),       # halo_fwd<5,128,64,2,true>+bal: window_exceeds_image; wgrad<128,128,32>+tab+slabs: multi_image_tile ragged wi ...
    (46, 41, 20, 32, 32, 5, 1),        # wgrad<32,128,64>+tab+slabs: ragged
    (255, 16, 16, 256, 512, 1, 2),     # fwd<128,128,32,2,0>+stats+tab: ragged; fwd<128,128,32,2,0>+tab: ragged
    (50, 26, 4, 64, 128, 5, 1),        # fwd<128,64,32,4,0>+bal+tab: window_exceeds_image
    (57, 51, 7, 64, 128, 5, 1),        # halo_fwd<5,128,64,2,true>+bal: tight_halo; wgrad<128,128,32>+tab+slabs: odd_width ragged
    (1, 128, 128, 64, 64, 5, 1),       # fwd<128,64,32,4,0>+bal+tab: one_image
    (60, 13, 5, 256, 512, 3, 1),       # wgrad<128,128,32>+tab+slabs: multi_image_tile odd_width
    (255, 51, 7, 32, 64, 5, 1),        # halo_fwd<5,128,64,2,false>: odd_width; halo_fwd<5,128,64,2,false>+stats: odd_width
    (8, 128, 128, 64, 64, 3, 1),       # fwd<128,64,16,4,0>+stats+tab: any; fwd<128,64,16,4,0>+tab: any
    (38, 101, 13, 64, 64, 5, 1),       # halo_fwd<5,128,64,2,false>: odd_width; halo_fwd<5,128,64,2,false>+stats: odd_width
    (100, 3, 10, 256, 256, 5, 1),      # halo_fwd<5,128,64,2,true>+bal: multi_image_tile
    (30, 13, 2, 512, 512, 5, 1),       # wgrad<128,128,32>+tab: window_exceeds_image
    (60, 13, 2, 256, 512, 5, 1),       # wgrad<128,128,32>+tab+slabs: window_exceeds_image
    (255, 26, 4, 128, 256, 5, 1),      # halo_fwd<5,128,64,2,false>: window_exceeds_image; halo_fwd<5,128,64,2,false>+stats: window_exceeds_image
]
