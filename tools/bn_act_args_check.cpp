// The argument checks of the dense-glue entries (csrc/bn_act.hip: the six bn_act / bn_sync entries, and bn_act_bwd_impl also
// through mccnn_linear_bn_act_bwd) run on the host alone: every call below is refused before a launch, so no GPU is needed
// and the host half of the library can be built with sanitizers. Each bad call must give its code; a call wrong in two ways
// the code of the check that comes first.
//   hipcc <the library's flags> -Xarch_host -fsanitize=address,undefined   (every csrc/*.hip -> one shared library)
//   clang++ -fsanitize=address,undefined -Iinclude tools/bn_act_args_check.cpp -L<dir> -l<library> -o bn_act_args_check
#include <cstdio>

#include "mccnn.h"

constexpr int n = 300, c = 8, world = 2, big = (1 << 24) + 1;
static int g_bad = 0;
static void expect(int got, int want, const char* what) {
    if (got != want) {
        std::printf("FAIL %s: %d, expected %d\n", what, got, want);
        ++g_bad;
    }
}

int main() {
    const unsigned long long all = 1ull << 32;
    alignas(16) static float x[n * c], y[n * c], v[6][c], saved[3 * c], parts[2 * 3 * c];
    static int meta[2];
    const size_t need = mccnn_bn_act_workspace_bytes(n, c);
    alignas(16) static char ws[1 << 16];
    expect(need > 0 && need <= sizeof ws, 1, "workspace query");
    void* odd = (char*)x + 2;   // a bf16 pointer off its 32-bit word
    const int BADARG = MCCNN_E_BADARG, TOOLARGE = MCCNN_E_TOOLARGE, WORKSPACE = MCCNN_E_WORKSPACE, SHAPE = MCCNN_E_SHAPE;

    auto fwd = [&](const void* x_, int xb, int n_, int c_, unsigned long long thr, void* y_, int yb, float* saved_, void* ws_,
                   size_t wsn, int training = 1) {
        return mccnn_bn_act_fwd_rows(x_, xb, n_, c_, v[0], v[1], v[2], v[3], 0.99f, 1e-3f, training, 1, thr, 1.f, 7u, y_, yb, saved_, ws_,
                                     wsn, nullptr);
    };
    expect(fwd(x, 0, 0, c, all, y, 0, saved, ws, need), BADARG, "fwd n = 0");
    expect(fwd(x, 0, n, 0, all, y, 0, saved, ws, need), BADARG, "fwd c = 0");
    expect(fwd(x, 0, n, c, 0, y, 0, saved, ws, need), BADARG, "fwd threshold 0");
    expect(fwd(x, 0, n, c, all + 1, y, 0, saved, ws, need), BADARG, "fwd threshold > 2^32");
    expect(fwd(nullptr, 0, n, c, all, y, 0, saved, ws, need), BADARG, "fwd x NULL");
    expect(fwd(x, 0, n, c, all, nullptr, 0, saved, ws, need), BADARG, "fwd y NULL");
    expect(fwd(x, 0, n, c, all, y, 0, nullptr, ws, need), BADARG, "fwd training without saved");
    expect(fwd(x, 2, n, c, all, y, 0, saved, ws, need), BADARG, "fwd x flag 2");
    expect(fwd(x, 0, n, c, all, y, -1, saved, ws, need), BADARG, "fwd y flag -1");
    expect(fwd(x, 1, n, 7, all, y, 0, saved, ws, need), SHAPE, "fwd bf16 x, odd c");
    expect(fwd(x, 0, n, 7, all, y, 1, saved, ws, need), SHAPE, "fwd bf16 y, odd c");
    expect(fwd(odd, 1, n, c, all, y, 0, saved, ws, need), SHAPE, "fwd bf16 x off a word");
    expect(fwd(x, 0, n, c, all, odd, 1, saved, ws, need), SHAPE, "fwd bf16 y off a word");
    expect(fwd(x, 0, n, c, all, y, 0, saved, ws, need - 1), WORKSPACE, "fwd short workspace");
    expect(fwd(x, 0, n, c, all, y, 0, saved, nullptr, need), WORKSPACE, "fwd workspace NULL");
    expect(fwd(x, 2, n, 7, all, y, 1, saved, nullptr, 0), BADARG, "fwd flag before shape before workspace");
    expect(fwd(x, 1, n, 7, all, y, 1, saved, nullptr, 0), SHAPE, "fwd shape before workspace");
    expect(fwd(x, 2, n, c, 0, y, 0, nullptr, ws, need, 0), BADARG, "fwd eval, threshold 0");
    expect(mccnn_bn_act_fwd(x, n, c, v[0], v[1], v[2], v[3], 0.99f, 1e-3f, 1, 1, all, 1.f, 7u, y, saved, ws, need - 1, nullptr), WORKSPACE,
           "the float32 forward, short workspace");

    auto bwd = [&](const void* x_, int xb, const void* dy_, int db, int n_, int c_, unsigned long long thr, void* dx_, float* dg, void* ws_,
                   size_t wsn) {
        return mccnn_bn_act_bwd_rows(x_, xb, dy_, db, n_, c_, v[0], v[1], saved, 1, thr, 1.f, 7u, dx_, dg, v[5], ws_, wsn, nullptr);
    };
    expect(bwd(x, 0, y, 0, 0, c, all, x, v[4], ws, need), BADARG, "bwd n = 0");
    expect(bwd(x, 0, y, 0, n, c, 0, x, v[4], ws, need), BADARG, "bwd threshold 0");
    expect(bwd(x, 0, nullptr, 0, n, c, all, x, v[4], ws, need), BADARG, "bwd dy NULL");
    expect(bwd(x, 0, y, 0, n, c, all, x, nullptr, ws, need), BADARG, "bwd dgamma NULL");
    expect(bwd(x, 0, y, 3, n, c, all, x, v[4], ws, need), BADARG, "bwd dy flag 3");
    expect(bwd(x, 1, y, 0, n, 7, all, nullptr, v[4], ws, need), SHAPE, "bwd bf16 x, odd c, no dx");
    expect(bwd(x, 0, odd, 1, n, c, all, x, v[4], ws, need), SHAPE, "bwd bf16 dy off a word");
    expect(bwd(x, 1, y, 0, n, c, all, odd, v[4], ws, need), SHAPE, "bwd bf16 dx off a word");
    expect(bwd(x, 0, y, 0, n, c, all, nullptr, v[4], ws, need - 1), WORKSPACE, "bwd short workspace, no dx");
    expect(bwd(x, 0, y, 0, n, c, all, x, v[4], nullptr, need), WORKSPACE, "bwd workspace NULL");
    expect(bwd(x, 1, y, 1, n, 7, all, x, v[4], nullptr, 0), SHAPE, "bwd shape before workspace");
    expect(mccnn_bn_act_bwd(x, y, n, c, v[0], v[1], saved, 1, all, 1.f, 7u, x, v[4], v[5], ws, 8, nullptr), WORKSPACE,
           "the float32 backward, short workspace");

    // bn_act_bwd_impl behind the linear layer's backward: that entry's own checks come first
    const size_t lneed = mccnn_linear_bn_act_workspace_bytes(n, 6, c);
    auto lin = [&](const void* dy_, int db, int cout, float* dw, float* dbeta, void* ws_, size_t wsn) {
        return mccnn_linear_bn_act_bwd(x, y, x, dy_, db, n, 6, cout, v[0], v[1], saved, 1, all, 1.f, 7u, nullptr, dw, v[3], v[4], dbeta, ws_,
                                       wsn, nullptr);
    };
    expect(lin(y, 0, c, nullptr, v[5], ws, lneed), BADARG, "linear bwd dw NULL");
    expect(lin(y, 0, c, y, nullptr, ws, lneed), BADARG, "linear bwd dbeta NULL");
    expect(lin(y, 2, c, y, v[5], ws, lneed), BADARG, "linear bwd dy flag 2");
    expect(lin(y, 1, 7, y, v[5], ws, lneed), SHAPE, "linear bwd bf16 dy, odd cout");
    expect(lin(odd, 1, c, y, v[5], ws, lneed), SHAPE, "linear bwd bf16 dy off a word");
    expect(lin(y, 0, c, y, v[5], ws, lneed - 1), WORKSPACE, "linear bwd short workspace");

    auto stats = [&](const void* x_, int xb, int n_, int c_, int rank, int world_, float* parts_, void* ws_, size_t wsn) {
        return mccnn_bn_sync_stats(x_, xb, n_, c_, rank, world_, parts_, ws_, wsn, nullptr);
    };
    expect(stats(x, 0, n, c, world, world, parts, ws, need), BADARG, "stats rank = world");
    expect(stats(x, 0, n, c, -1, world, parts, ws, need), BADARG, "stats rank -1");
    expect(stats(x, 0, n, c, 0, 0, parts, ws, need), BADARG, "stats world 0");
    expect(stats(x, 0, big, c, 0, world, parts, ws, need), TOOLARGE, "stats n > 2^24");
    expect(stats(nullptr, 2, big, c, 0, world, nullptr, nullptr, 0), TOOLARGE, "stats n > 2^24 before everything else");
    expect(stats(nullptr, 0, n, c, 0, world, parts, ws, need), BADARG, "stats x NULL");
    expect(stats(x, 0, n, c, 0, world, nullptr, ws, need), BADARG, "stats parts NULL");
    expect(stats(x, 2, n, c, 0, world, parts, ws, need), BADARG, "stats flag 2");
    expect(stats(x, 1, n, 7, 0, world, parts, ws, need), SHAPE, "stats bf16 x, odd c");
    expect(stats(odd, 1, n, c, 0, world, parts, nullptr, 0), SHAPE, "stats bf16 x off a word, before workspace");
    expect(stats(x, 0, n, c, 0, world, parts, ws, need - 1), WORKSPACE, "stats short workspace");
    expect(stats(x, 0, n, c, 0, world, parts, nullptr, need), WORKSPACE, "stats workspace NULL");

    auto apply = [&](int rank, int world_, const float* parts_, unsigned long long thr, void* y_, int yb, float* saved_, int* meta_,
                     int c_ = c) {
        return mccnn_bn_sync_apply(x, 0, n, c_, rank, world_, parts_, v[0], v[1], v[2], v[3], 0.99f, 1e-3f, 1, thr, 1.f, 7u, y_, yb, saved_,
                                   meta_, nullptr);
    };
    expect(apply(world, world, parts, all, y, 0, saved, meta), BADARG, "apply rank = world");
    expect(apply(0, world, parts, 0, y, 0, saved, meta), BADARG, "apply threshold 0");
    expect(apply(0, world, parts, all + 1, y, 0, saved, meta), BADARG, "apply threshold > 2^32");
    expect(apply(0, world, nullptr, all, y, 0, saved, meta), BADARG, "apply parts NULL");
    expect(apply(0, world, parts, all, y, 0, nullptr, meta), BADARG, "apply saved NULL");
    expect(apply(0, world, parts, all, y, 0, saved, nullptr), BADARG, "apply meta NULL");
    expect(apply(0, world, parts, all, y, 2, saved, meta), BADARG, "apply y flag 2");
    expect(apply(0, world, parts, all, y, 1, saved, meta, 7), SHAPE, "apply bf16 y, odd c");
    expect(apply(0, world, parts, all, odd, 1, saved, meta), SHAPE, "apply bf16 y off a word");

    auto sums = [&](int rank, const void* dy_, int db, int c_, unsigned long long thr, const int* meta_, float* dg, void* ws_, size_t wsn,
                    int n_ = n) {
        return mccnn_bn_sync_bwd_sums(x, 0, dy_, db, n_, c_, rank, world, v[0], v[1], saved, meta_, 1, thr, 1.f, 7u, parts, dg, v[5], ws_,
                                      wsn, nullptr);
    };
    expect(sums(world, y, 0, c, all, meta, v[4], ws, need), BADARG, "sums rank = world");
    expect(sums(0, y, 0, c, all, meta, v[4], ws, need, big), TOOLARGE, "sums n > 2^24");
    expect(sums(0, y, 0, c, 0, meta, v[4], ws, need), BADARG, "sums threshold 0");
    expect(sums(0, y, 0, c, all, nullptr, v[4], ws, need), BADARG, "sums meta NULL");
    expect(sums(0, y, 0, c, all, meta, nullptr, ws, need), BADARG, "sums dgamma NULL");
    expect(sums(0, y, 2, c, all, meta, v[4], ws, need), BADARG, "sums dy flag 2");
    expect(sums(0, y, 1, 7, all, meta, v[4], ws, need), SHAPE, "sums bf16 dy, odd c");
    expect(sums(0, odd, 1, c, all, meta, v[4], nullptr, 0), SHAPE, "sums bf16 dy off a word, before workspace");
    expect(sums(0, y, 0, c, all, meta, v[4], ws, 8), WORKSPACE, "sums short workspace");

    auto dx = [&](int rank, int n_, int xb, int c_, const void* dy_, int db, unsigned long long thr, void* dx_, float* dg) {
        return mccnn_bn_sync_bwd_dx(x, xb, dy_, db, n_, c_, rank, world, v[0], v[1], parts, saved, meta, 1, thr, 1.f, 7u, dx_, dg, nullptr);
    };
    expect(dx(-1, n, 0, c, y, 0, all, y, v[4]), BADARG, "dx rank -1");
    expect(dx(0, big, 0, c, y, 0, all, y, v[4]), TOOLARGE, "dx n > 2^24");
    expect(dx(0, n, 0, c, y, 0, 0, y, v[4]), BADARG, "dx threshold 0");
    expect(dx(0, n, 0, c, y, 0, all, nullptr, nullptr), BADARG, "dx neither dx nor dgamma");
    expect(dx(0, n, 0, c, nullptr, 0, all, y, v[4]), BADARG, "dx dy NULL");
    expect(dx(0, n, 2, c, y, 0, all, y, v[4]), BADARG, "dx x flag 2");
    expect(dx(0, n, 1, 7, y, 0, all, nullptr, v[4]), SHAPE, "dx bf16 x, odd c, no dx");
    expect(dx(0, n, 0, c, odd, 1, all, y, v[4]), SHAPE, "dx bf16 dy off a word");
    expect(dx(0, n, 1, c, y, 0, all, odd, v[4]), SHAPE, "dx bf16 dx off a word");

    expect((int)mccnn_debug_launch_count(), 0, "launches");
    std::printf(g_bad ? "%d check(s) failed\n" : "bn_act argument checks ok\n", g_bad);
    return g_bad ? 1 : 0;
}
