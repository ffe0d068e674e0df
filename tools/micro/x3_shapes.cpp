// x3_shapes.cpp -- prints the split kernels' host shape queries over a grid, to compare two builds.
// Links the split-kernel objects and calls no HIP API:
//   g++ -std=c++17 -c tools/micro/x3_shapes.cpp -o build/x3_shapes.o
//   hipcc build/x3_shapes.o build/rollout_x3.o build/rollout_x3_plain.o build/rollout_pp.o -o tools/micro/x3_shapes
// (profiles/x3_split_shapes.txt is its output; it did not change when rollout_x3.hip was split.)
#include <cstddef>
#include <cstdio>

#include "../../bc_mpc_amd/csrc/shapes.h"

int main() {
    using namespace bcmpc;
    const int HID[] = {64, 128, 256, 512, 768, 1024}, NCS[] = {1, 2, 4, 8}, NWS[] = {2, 4, 8, 16}, LS[] = {1, 2, 3};
    const int SA[][2] = {{20, 6}, {17, 6}, {1, 1}, {26, 6}, {20, 12}}, AS[] = {6, 1, 12}, POL[] = {0, 128};
    std::printf("# grid: nc 1 2 4 8 | nw 2 4 8 16 | L 1 2 3 | A 6 1 12 | (S,A) (20,6) (17,6) (1,1) (26,6) (20,12) | "
                "policy off, 128 (2 layers) | ak 0..3; the innermost index varies fastest, ';' closes one\n");
    for (int h : HID) {
        std::printf("hidden %d: x3_waves %d  x3_max_nc %d  x3_policy_ok[nc]", h, x3_waves(h), x3_max_nc(h));
        for (int nc : NCS) std::printf(" %d", (int)x3_policy_ok(h, nc));
        std::printf("  x3_f16_layout_ok[nc][nw]");
        for (int nc : NCS) {
            for (int nw : NWS) std::printf(" %d", (int)x3_f16_layout_ok(h, nc, nw));
            std::printf(";");
        }
        std::printf("\n");
        for (int l : LS)
            for (int nc : NCS) {
                std::printf("hidden %d L %d nc %d: x3_lds[A][policy][ak]", h, l, nc);
                for (int A : AS) {
                    for (int php : POL)
                        for (int ak = 0; ak < 4; ++ak) std::printf(" %zu", x3_lds(h, l, nc, A, php ? 2 : 0, php, ak));
                    std::printf(";");
                }
                std::printf("\nhidden %d L %d nc %d: x3_f16_lds[A][nw]", h, l, nc);
                for (int A : AS) {
                    for (int nw : NWS) std::printf(" %zu", x3_f16_lds(h, l, nc, nw, A));
                    std::printf(";");
                }
                std::printf("\n");
            }
        for (const auto& sa : SA) {
            std::printf("hidden %d S %d A %d: x3_pp3_lds %zu  x3_pp_ok[L]", h, sa[0], sa[1], x3_pp3_lds(h, sa[0], sa[1]));
            for (int l : LS) std::printf(" %d", (int)x3_pp_ok(h, l, sa[0], sa[1]));
            std::printf("  x3_pp3_ok[L]");
            for (int l : LS) std::printf(" %d", (int)x3_pp3_ok(h, l, sa[0], sa[1]));
            std::printf("\n");
        }
    }
    return 0;
}
