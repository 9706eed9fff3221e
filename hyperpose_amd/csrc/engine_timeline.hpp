// engine_timeline.hpp — the HP_CONV_DBG / HP_BN_DBG / HP_CHAIN_DBG / HP_SEP_DBG / HP_DIRECT_DBG block timelines as text.
//
// The engine launches a step's kernel once more with a zeroed stamp buffer (engine.cpp: hp_engine::trace_step) and hands the stamps it copied
// back to print_timeline.  Everything here is host text formatting with no HIP call: tests/cpp/engine_timeline.cpp feeds it synthetic buffers
// and compares the text with tests/golden/engine_timelines.txt, which tools/*_timeline.py users diff.
#pragma once

#include <cstddef>
#include <cstdio>

namespace hp {

enum class timeline_kind {
    conv,   // fp16 pixel-block GEMM (conv1x1_big_kernel): consumer / producer wavefront of block 0
    bneck,  // conv_bottleneck.hip: block 0's phases, then (start, end) of the first 1024 blocks
    chain,  // conv_chain.hip: block 0's phases
    sep,    // sepconv_kernel: block 0, (start, end) of the first 1024 blocks, wavefront 4 of block 1
    wino,   // conv32_winograd.hip: block (1, 0), thread 0
    direct, // conv32_direct.hip: block (1, 0), thread 0
    conv32, // conv32_kernel: block 9, thread 0, then every block's residency
};

// the few numbers the texts quote (a kind prints the ones it has)
struct timeline_header {
    int layer;
    int cin, cout; // sep: cin = the block's channels
    int kh, kw;
    int tile;          // the step's tile or variant code
    int blocks_per_cu; // wino: what the runtime grants the kernel
};

size_t timeline_words(timeline_kind k); // 8-byte stamps the kind's kernels write at most
void print_timeline(FILE* f, timeline_kind k, const timeline_header& hd, const unsigned long long* stamps); // stamps[timeline_words(k)]

} // namespace hp
