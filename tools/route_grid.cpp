// Host-only walk of the Conv1D routing functions (rag4dyg_amd/csrc/conv1d_route.h) over the grid of
// tests/test_host_conv1d_route.py (and the head's precision value 2 of tests/test_host_train_bf16_head.py), for a sanitizer build on a machine without a GPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/route_grid.cpp -o route_grid && ./route_grid
// Prints the number of points per route; any sanitizer report ends it with a non-zero status.
#include <initializer_list>
#include <stdio.h>
#include "../rag4dyg_amd/csrc/conv1d_route.h"

int r4d::g_gemm_split3 = 1;

int main() {
    using namespace r4d;
    const int Ms[] = {1, 32, 33, 4096, 31, 32, 390, 4100}, Ks[] = {48, 64, 256, 512}, Ns[] = {64, 128, 192, 256, 1536};
    long long hits[ROUTE_COUNT] = {0}, n = 0;
    for (int mode = 0; mode <= 2; ++mode) {
        g_gemm_split3 = mode;
        for (int kind = 0; kind < 6; ++kind)
            for (int bf16 = 0; bf16 <= 2; ++bf16)                     // 2: the LM head under its own switch (kinds 2, 4, 5)
                for (unsigned have = 0; have < 32; ++have)
                    for (int epi = 0; epi < 8; ++epi)
                        for (int mi = 0; mi < (kind == 5 ? 8 : 4); ++mi)
                            for (int K : Ks)
                                for (int N : Ns) {
                                    const int r = conv1d_route_query(kind, Ms[mi], K, N, epi, have, bf16);
                                    if (r < 0 || r >= ROUTE_COUNT) { printf("bad route %d\n", r); return 1; }
                                    ++hits[r]; ++n;
                                }
    }
    for (int mode = 0; mode <= 2; ++mode) {                      // empty and negative shapes: -1, whatever the kind and mode
        g_gemm_split3 = mode;
        for (int kind = 0; kind < 6; ++kind)
            for (int bf16 = 0; bf16 <= 2; ++bf16)                     // 2: the LM head under its own switch (kinds 2, 4, 5)
                for (int bad : {0, -1, -128, -2147483647 - 1}) {
                    if (conv1d_route_query(kind, bad, 128, 256, 0, 31, bf16) != -1 || conv1d_route_query(kind, 390, bad, 256, 0, 31, bf16) != -1 ||
                        conv1d_route_query(kind, 390, 128, bad, 0, 31, bf16) != -1) { printf("empty shape not refused\n"); return 1; }
                    (void)wgrad_route(bad, 256, 390, 128, 256, bf16); (void)wgrad_route(128, bad, 390, 128, 256, bf16);
                    (void)wgrad_route(128, 256, bad, 128, 256, bf16); (void)tn_splits(bad, bad, bad);
                }
    }
    if (conv1d_route_query(6, 32, 256, 256, 0, 0, 0) != -1 || gemm_route_name(-1)[0] != 'u' || gemm_route_name(ROUTE_COUNT)[0] != 'u') return 1;
    for (int r = 0; r < ROUTE_COUNT; ++r) printf("%-12s %lld\n", gemm_route_name(r), hits[r]);
    printf("%lld points\n", n);
    return 0;
}
