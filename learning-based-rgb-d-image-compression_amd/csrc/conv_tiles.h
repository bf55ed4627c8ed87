// The tile forms the convolution dispatch instantiates, as list macros: X(WM, WN, MT, NT) once per workgroup tile of
// TM = 16 * MT * WM couts x TP = 16 * NT * WN pixels.  launch_conv_main (conv_mfma.hip) and launch_conv_blk
// (conv_mfma_blk.hip) expand them into their dispatch chains, conv_tile_list (rgbd_debug_tile_list) into text, so the
// tests sweep exactly what is compiled (tests/test_gpu_conv_tiles.py) and a tile added here is tested without another edit.
//
// Every tile of a family exists with 64 channels per stage (kc 64), with 16 register-staged (kc 16, staging mode 0) and with
// 16 direct-to-LDS double-buffered under an LDS cap of 78 / 52 / 38 KiB (modes 1 / 2 / 3); the tiles with whole waves of
// patch slots (TP % 64 == 0) also as a ring of four / three direct-to-LDS stages (modes 4 / 5, single-tap layers).
#pragma once

// in both families, with ring forms
#define RGBD_TILES_RING_BOTH(X)                                                                            \
    X(2, 2, 2, 8) X(2, 2, 1, 8) X(1, 4, 3, 4) X(1, 4, 2, 4) X(1, 4, 1, 4)                                  \
    X(2, 2, 4, 4) X(2, 2, 3, 4) X(2, 2, 2, 4) X(2, 2, 1, 4)                                                \
    X(2, 2, 5, 2) X(2, 2, 4, 2) X(2, 2, 3, 2) X(2, 2, 2, 2) X(2, 2, 1, 2)                                  \
    X(1, 4, 3, 2) X(1, 4, 2, 2) X(1, 4, 1, 2) X(1, 4, 3, 1) X(1, 4, 2, 1) X(1, 4, 1, 1)
// single-chain only: more than 16 result tiles per wave leave no room for the second accumulator set of the blocked kernels
#define RGBD_TILES_RING_MAIN_ONLY(X) X(2, 2, 3, 8) X(2, 2, 5, 4)
// 32-pixel tiles: half a wave of patch slots, no ring form
#define RGBD_TILES_NO_RING(X) X(2, 2, 5, 1) X(2, 2, 4, 1) X(2, 2, 3, 1) X(2, 2, 2, 1) X(2, 2, 1, 1)

// single-chain kernels (conv_mfma.hip): 27 tiles, 22 of them with ring forms
#define RGBD_TILES_MAIN_RING(X) RGBD_TILES_RING_MAIN_ONLY(X) RGBD_TILES_RING_BOTH(X)
#define RGBD_TILES_MAIN(X) RGBD_TILES_MAIN_RING(X) RGBD_TILES_NO_RING(X)
// blocked-accumulation kernels (conv_mfma_blk.hip): 25 tiles, 20 of them with ring forms
#define RGBD_TILES_BLK_RING(X) RGBD_TILES_RING_BOTH(X)
#define RGBD_TILES_BLK(X) RGBD_TILES_BLK_RING(X) RGBD_TILES_NO_RING(X)
