// Host-side check of the BatchNorm entry points' argument validation and workspace layout, for a sanitizer build.
// Stand-alone (its own main), CPU only: every call below is rejected before anything touches a device.
//
//   cd ssl4gie_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../../tools/bn_abi_host_check.cpp resnet_ops.hip norm.hip -o /tmp/bn_abi_host_check
//   /tmp/bn_abi_host_check        # prints one summary line; the sanitizers report nothing; exit status 0
#include <cstdio>
#include <vector>

#include "prof.h"
#include "ssl4gie_hip.h"

ProfState g_prof = {false, 0, 0, nullptr, nullptr, nullptr};  // the library's lives in engine.hip (profiler off)

namespace {
int failures = 0, calls = 0;
void expect_earg(int rc, const char* what, unsigned bits) {
    ++calls;
    if (rc != SSL4GIE_EARG) {
        ++failures;
        std::fprintf(stderr, "%s (pointers 0x%x): rc %d, expected SSL4GIE_EARG\n", what, bits, rc);
    }
}
}  // namespace

int main() {
    const long long rows = 4;
    const int C = 8;
    const size_t ws_bytes = ssl4gie_bn_workspace_bytes(rows, C);
    // the layout the five functions carve up: [coef 3C][partials parts x 2C][sums 2C][pivot C] + 64 x 2C of fold room,
    // parts >= 64
    if (ws_bytes != (size_t)(3 + 2 * 64 + 2 + 1 + 2 * 64) * C * sizeof(float)) {
        std::fprintf(stderr, "ssl4gie_bn_workspace_bytes(4, 8) = %zu\n", ws_bytes);
        return 1;
    }
    for (long long r : {1LL, 1LL << 20, 1LL << 26}) {
        for (int c : {8, 64, 2048}) {
            long long p = ((r * c) >> 16) / ((c + 511) / 512);
            p = p < 64 ? 64 : (p > 1024 ? 1024 : p);
            if (ssl4gie_bn_workspace_bytes(r, c) != (size_t)(3 + 2 * p + 2 + 1 + 2 * 64) * c * sizeof(float)) {
                std::fprintf(stderr, "ssl4gie_bn_workspace_bytes(%lld, %d) = %zu\n", r, c, ssl4gie_bn_workspace_bytes(r, c));
                return 1;
            }
        }
    }
    // one real host buffer per pointer argument
    std::vector<std::vector<unsigned char>> buf(13, std::vector<unsigned char>(ws_bytes));
    auto P = [&](unsigned bits, int i) -> void* { return (bits >> i) & 1u ? buf[i].data() : nullptr; };
    auto F = [&](unsigned bits, int i) -> float* { return (float*)P(bits, i); };
    auto U = [&](unsigned bits, int i) -> unsigned char* { return (unsigned char*)P(bits, i); };

    // every subset of the pointers, every selector and dtype, with a channel count (12) or a row count (0) that no
    // form accepts: each combination runs through the validator and comes back as an argument error
    for (int bad = 0; bad < 2; ++bad) {
        const long long r = bad ? 0 : rows;
        const int c = bad ? C : 12;
        for (int sel = -1; sel <= 4; ++sel) {
            for (int dt = 0; dt <= 2; ++dt) {
                for (unsigned b = 0; b < (1u << 13); ++b) {
                    // coefficients of given statistics (FROM_STATS without y) check only C > 0: not rejected here
                    if (sel == SSL4GIE_BN_FROM_STATS && !((b >> 5) & 1u)) continue;
                    for (int relu = 0; relu < 2; ++relu)
                        expect_earg(ssl4gie_bn_fwd(sel, P(b, 0), F(b, 1), 2, F(b, 2), F(b, 3), P(b, 4), P(b, 5), U(b, 6), F(b, 7),
                                                   F(b, 8), F(b, 9), F(b, 10), F(b, 11), 0.1f, 1e-5f, relu, F(b, 12), dt, r, c,
                                                   nullptr), "bn_fwd", b);
                }
                for (unsigned b = 0; b < (1u << 12); ++b)
                    expect_earg(ssl4gie_bn_bwd(P(b, 0), sel, P(b, 1), P(b, 2), F(b, 3), F(b, 4), F(b, 5), F(b, 6), P(b, 7), P(b, 8),
                                               F(b, 9), F(b, 10), 0, F(b, 11), dt, r, c, nullptr), "bn_bwd", b);
                for (unsigned b = 0; b < (1u << 10); ++b) {
                    expect_earg(ssl4gie_bn_bwd_reduce(P(b, 0), sel, P(b, 1), P(b, 2), F(b, 3), F(b, 4), F(b, 5), F(b, 6), P(b, 7),
                                                      F(b, 8), F(b, 9), dt, r, c, nullptr), "bn_bwd_reduce", b);
                    expect_earg(ssl4gie_bn_bwd_apply(P(b, 0), sel, P(b, 1), P(b, 2), F(b, 3), F(b, 4), F(b, 5), F(b, 6), F(b, 7),
                                                     0.25f, P(b, 8), F(b, 9), dt, r, c, nullptr), "bn_bwd_apply", b);
                }
            }
        }
        for (int dt = 0; dt <= 2; ++dt)
            for (unsigned b = 0; b < (1u << 5); ++b)
                expect_earg(ssl4gie_bn_stats(P(b, 0), F(b, 1), 2, F(b, 2), F(b, 3), F(b, 4), dt, r, c, nullptr), "bn_stats", b);
    }

    // combinations no kernel serves, at a shape every form accepts
    const unsigned all = ~0u;
    float* ws = F(all, 12);
    void *x = P(all, 0), *y = P(all, 5), *dy = P(all, 4), *dx = P(all, 7), *dres = P(all, 8), *mask = P(all, 6);
    float *mean = F(all, 8), *rstd = F(all, 9), *coef = F(all, 7), *beta = F(all, 3), *sums = F(all, 10), *part = F(all, 1);
    unsigned char* bits = U(all, 6);
    const int F32 = SSL4GIE_F32, BF16 = SSL4GIE_BF16;
    // forward: y == NULL with FROM_X; relu_bits with fp32, without ReLU, or behind a statistics pass; FROM_COEF without
    // coef; FROM_STATS with running statistics; partials with another source and PARTIALS without them
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_X, x, 0, 0, 0, 0, 0, nullptr, 0, coef, mean, rstd, 0, 0, .1f, 1e-5f, 0, ws, BF16, rows, C, 0), "fwd X, no y", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_PARTIALS, x, part, 2, 0, 0, 0, y, bits, 0, mean, rstd, 0, 0, .1f, 1e-5f, 1, ws, F32, rows, C, 0), "fwd bits fp32", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_PARTIALS, x, part, 2, 0, 0, 0, y, bits, 0, mean, rstd, 0, 0, .1f, 1e-5f, 0, ws, BF16, rows, C, 0), "fwd bits, relu 0", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_X, x, 0, 0, 0, 0, 0, y, bits, 0, mean, rstd, 0, 0, .1f, 1e-5f, 1, ws, BF16, rows, C, 0), "fwd X bits", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_COEF, x, 0, 0, 0, 0, 0, y, bits, nullptr, 0, 0, 0, 0, .1f, 1e-5f, 1, 0, BF16, rows, C, 0), "fwd COEF, no coef", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_STATS, x, 0, 0, 0, 0, 0, y, 0, 0, mean, rstd, sums, sums, .1f, 1e-5f, 1, ws, BF16, rows, C, 0), "fwd STATS running", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_X, x, part, 2, 0, 0, 0, y, 0, 0, mean, rstd, 0, 0, .1f, 1e-5f, 1, ws, BF16, rows, C, 0), "fwd X partial", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_PARTIALS, x, 0, 2, 0, 0, 0, y, 0, 0, mean, rstd, 0, 0, .1f, 1e-5f, 1, ws, BF16, rows, C, 0), "fwd PARTIALS none", 0);
    expect_earg(ssl4gie_bn_fwd(SSL4GIE_BN_FROM_PARTIALS, x, part, 0, 0, 0, 0, y, 0, 0, mean, rstd, 0, 0, .1f, 1e-5f, 1, ws, BF16, rows, C, 0), "fwd parts 0", 0);
    expect_earg(ssl4gie_bn_stats(x, part, 2, mean, rstd, ws, BF16, rows, C, 0), "stats x and partial", 0);
    // backward: BITS with fp32 / without dres / in the apply half; MASK_X with a mask tensor or a residual gradient;
    // MASK_Y without y; beta outside MASK_X; gamma in a reduce half that does not rebuild the mask
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_BITS, mask, x, 0, 0, mean, rstd, dx, dres, 0, 0, 0, ws, F32, rows, C, 0), "bwd BITS fp32", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_BITS, mask, x, 0, 0, mean, rstd, dx, nullptr, 0, 0, 0, ws, BF16, rows, C, 0), "bwd BITS no dres", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_X, mask, x, 0, beta, mean, rstd, dx, 0, 0, 0, 0, ws, BF16, rows, C, 0), "bwd X mask", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_X, 0, x, 0, beta, mean, rstd, dx, dres, 0, 0, 0, ws, BF16, rows, C, 0), "bwd X dres", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_X, 0, x, 0, beta, nullptr, rstd, dx, 0, 0, 0, 0, ws, BF16, rows, C, 0), "bwd X no mean", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_Y, nullptr, x, 0, 0, mean, rstd, dx, 0, 0, 0, 0, ws, BF16, rows, C, 0), "bwd Y no y", 0);
    expect_earg(ssl4gie_bn_bwd(dy, SSL4GIE_BN_MASK_Y, mask, x, 0, beta, mean, rstd, dx, 0, 0, 0, 0, ws, BF16, rows, C, 0), "bwd Y beta", 0);
    expect_earg(ssl4gie_bn_bwd_reduce(dy, SSL4GIE_BN_MASK_BITS, mask, x, 0, 0, mean, rstd, nullptr, sums, ws, BF16, rows, C, 0), "reduce BITS no dres", 0);
    expect_earg(ssl4gie_bn_bwd_reduce(dy, SSL4GIE_BN_MASK_BITS, mask, x, 0, 0, mean, rstd, dres, sums, ws, F32, rows, C, 0), "reduce BITS fp32", 0);
    expect_earg(ssl4gie_bn_bwd_reduce(dy, SSL4GIE_BN_MASK_Y, mask, x, beta, 0, mean, rstd, 0, sums, ws, BF16, rows, C, 0), "reduce Y gamma", 0);
    expect_earg(ssl4gie_bn_bwd_reduce(dy, SSL4GIE_BN_MASK_X, 0, x, 0, 0, mean, rstd, dres, sums, ws, BF16, rows, C, 0), "reduce X dres", 0);
    expect_earg(ssl4gie_bn_bwd_apply(dy, SSL4GIE_BN_MASK_BITS, mask, x, 0, 0, mean, rstd, sums, .25f, dx, ws, BF16, rows, C, 0), "apply BITS", 0);
    expect_earg(ssl4gie_bn_bwd_apply(dy, SSL4GIE_BN_MASK_X, mask, x, 0, 0, mean, rstd, sums, .25f, dx, ws, BF16, rows, C, 0), "apply X mask", 0);
    expect_earg(ssl4gie_bn_bwd_apply(dy, SSL4GIE_BN_MASK_NONE, 0, x, 0, 0, mean, rstd, nullptr, .25f, dx, ws, BF16, rows, C, 0), "apply no sums", 0);

    std::printf("bn_abi_host_check: %d rejected calls, %d not rejected\n", calls, failures);
    return failures ? 1 : 0;
}
