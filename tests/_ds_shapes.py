"""Launch shapes of the depthwise-separable topologies A_ds / B_ds -- importable without the library, so that the host-only
coverage test (tests/test_dsnet_reference_cpu.py) can hold the lists against the plan walk of the whole search space."""

#: pointwise halves, (B, H, W, C_in, C_out, KS = 1, stride = 1): compared with float64 through the trainer's launch path by
#: tests/test_gpu_ds_shapes.py.  Together they produce every launch-path variant (cmoop_conv_launch_plan: forward with and
#: without the statistics epilogue, data gradient, weight gradient) that a pointwise layer of any gene takes at 101 x 40
#: features, batch 64 and 37.  Behind each case: the variants it was picked for.
DS_POINTWISE_CONVS = [
    (37, 101, 40, 16, 16, 1, 1),     # fwd<128,16,16,4,0>(+stats)+tab, wgrad<16,64,64>+tab+slabs
    (37, 101, 40, 64, 64, 1, 1),     # fwd<128,64,16,4,0>(+stats)+tab, wgrad<64,64,64>+tab+slabs
    (64, 51, 20, 16, 32, 1, 1),      # fwd<128,32,16,4,0>(+stats)+tab, dgrad fwd<128,16,32,4,0>+tab, wgrad<32,64,64>+tab+slabs
    (37, 51, 20, 16, 32, 1, 1),      # fwd<64,32,16,4,0>(+stats)+tab, dgrad fwd<64,16,32,4,0>+tab
    (64, 51, 20, 32, 32, 1, 1),      # fwd<128,32,32,4,1>(+stats)+tab (LDS-DMA operand loads)
    (37, 51, 20, 32, 32, 1, 1),      # fwd<64,32,32,4,0>(+stats)+tab
    (64, 51, 20, 32, 64, 1, 1),      # fwd<128,64,32,4,0>(+stats)+tab
    (64, 51, 20, 64, 128, 1, 1),     # fwd<128,128,32,2,0>(+stats)+tab, wgrad<128,64,32>+tab+slabs
    (37, 26, 10, 32, 64, 1, 1),      # fwd<64,64,32,2,0>(+stats)+tab
    (37, 13, 5, 256, 512, 1, 1),     # dgrad fwd<128,128,32,2,0>+sk+tab (split-K), the deepest stage
]

#: depthwise halves, (H, W, C, K): every geometry cmoop_plan_dwconvs lists over the search space at 101 x 40 features
DS_DWCONVS = [(H, W, C, K)
              for (H, W), chans in (((101, 40), (16, 32, 64)), ((51, 20), (16, 32, 64, 128)), ((26, 10), (32, 64, 128, 256)),
                                    ((13, 5), (64, 128, 256, 512)))
              for C in chans for K in (3, 5)]
