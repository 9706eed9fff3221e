// Host-only: the profile tile code csrc/conv_pick.hpp gives a dense fp16 layer on given maps - what a GPU test expects of the engine
// without asking the engine (tests/test_engine_tiny_maps_gpu.py).  The layer is described as conv_pick.cpp's table describes one
// (make_case: the engine's padding of Cin / Cout, TF "SAME" geometry), with the weight layout the engine would pack for it.
//   conv_pick_at.bin K Cin Cout B stride dil residual H W [H W ...]   prints one tile code per map
#define main conv_pick_table_main
#include "conv_pick.cpp"
#undef main

#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 10 || (argc - 8) % 2) {
        std::printf("usage: %s K Cin Cout B stride dil residual H W [H W ...]\n", argv[0]);
        return 2;
    }
    int a[7];
    for (int i = 0; i < 7; ++i)
        a[i] = std::atoi(argv[1 + i]);
    for (int i = 8; i + 1 < argc; i += 2) {
        const geom g{a[0], a[0], a[1], a[2], std::atoi(argv[i]), std::atoi(argv[i + 1]), a[3], a[4], a[5], 0, a[6] ? 4 : 0, 0, 0};
        conv_params p = make_case(g);
        p.w_layout = pick::weight_layout(p); // (lower16_conv: the launcher says which packing its kernel for this shape reads)
        std::printf("%d\n", pick::tile(p));
    }
    return 0;
}
