// conv_route_check -- what mccnn_conv_prepare reports (pieces to attach, scratch, bytes of `saved`) over a lattice of layer
// shapes, lists, flags and geometries, computed on the HOST: no GPU, no launch. mccnn_conv_prepare itself wants a built
// geometry, so this program is the executor's own translation unit (csrc/exec.hip, included below) with a main(): it hands
// requirements() geometries that were never built -- sizes and attached pieces filled in by hand, no buffer is ever
// dereferenced -- and links libmccnn_hip.so for the size queries of the kernels.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Iinclude -Imccnn_amd/csrc \
//         tools/conv_route_check.hip -Lmccnn_amd/lib -l:libmccnn_hip.so -Wl,-rpath,$PWD/mccnn_amd/lib -o conv_route_check
//   ./conv_route_check            the table tests/golden/conv_route_req.txt holds (tests/test_conv_route_cpu.py compares them
//                                 byte for byte)
//   ./conv_route_check --routes   the same with the route record of every line in front of its sizes
//
// The golden table was written once, at the last commit before the route record, by this program's first form, which called
// that commit's requirements(geometry, shape, feats, backward, flags, e) (NOTES.md "One route decision per convolution layer").
//
// One line per (shape, list, direction, pieces, alignment): which of the line's distinct answers each of flags = 0..7 gets
// (eight digits), then those answers in the order of their first appearance.
//   fin fout combin bf16 | n m e | b<backward> p<pieces> a<aligned> : 01010101 : rc mask need[0..3] ws saved ; ...
// pieces: 0 nothing attached, 1 plans / transposed list / records attached but not built, 2 built as well.
#include "../mccnn_amd/csrc/exec.hip"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace {

struct ListCase { int n, m, e; };
// both sides of 500 000 edges, of 65 536 points, of 16 edges per point, of the unsorted limit (32 768 points); a pooling
// level (m < n), an empty list, a level without centres
const ListCase LISTS[] = {{1878, 1878, 155372}, {909, 300, 21946},    {41000, 41000, 500000}, {41000, 41000, 500001},
                          {32768, 8192, 400000}, {32769, 8192, 400000}, {65535, 65535, 1500000}, {65536, 16384, 1500000},
                          {3495, 3495, 1349070}, {131072, 131072, 2097151}, {131072, 131072, 2097152}, {600, 600, 0}, {600, 0, 0}};
// every (Fin, Fout) of tests/combin_cases.py (STATIC, GENERIC, WIDE), refused ones included
const int COMBIN[][2] = {{2, 16}, {2, 17}, {2, 21}, {3, 6}, {3, 5}, {3, 7}, {3, 10}, {3, 11}, {3, 15}, {4, 5}, {4, 8}, {4, 11}, {4, 12},
                         {5, 1}, {8, 1}, {5, 3}, {5, 7}, {6, 3}, {7, 5}, {7, 7}, {9, 1}, {9, 8}, {12, 2}, {16, 3}, {20, 2}, {20, 1},
                         {4, 100}, {5, 80}, {4, 102}, {5, 81}, {6, 67}, {4, 128}, {8, 64}, {1, 400}, {1, 408}, {1, 512}, {1, 520},
                         {1, 8}, {1, 64}};
const int DEPTHWISE[] = {8, 64, 256, 7, 136};

mccnn_geometry fake_geometry(const ListCase& L, int pieces) {
    mccnn_geometry g;
    g.n = L.n; g.m = L.m; g.e = g.e_cap = L.e; g.B = 2; g.built = true;
    if (pieces) {
        char* somewhere = reinterpret_cast<char*>(uintptr_t(4096));  // (never read)
        const size_t plenty = size_t(1) << 40;
        g.plan[0].buf = g.plan[1].buf = g.tl_buf = g.rec_buf = somewhere;
        g.plan[0].bytes = g.plan[1].bytes = g.tl_bytes = g.rec_bytes = plenty;
        g.tl_built = pieces == 2;
        g.plan[0].built = g.plan[1].built = pieces == 2;
    }
    return g;
}

std::string sizes(const ListCase& L, const Shape& s, int backward, int pieces, bool aligned, int flags, bool routes) {
    mccnn_geometry g = fake_geometry(L, pieces);
    Req r;
    char buf[512];
    int at = 0;
    const ConvRoute rt = conv_route(L.n, L.m, L.e, s, flags, aligned);
    if (routes)
        at = snprintf(buf, sizeof buf, "[rows %d%d unsorted %d family %d f1 %d rows_bytes %zu state_bytes %zu tlist %d] ", (int)rt.rows_fwd,
                      (int)rt.rows_bwd, (int)rt.unsorted, rt.family, (int)rt.f1, rt.rows_bytes, rt.state_bytes, rt.tlist);
    const int rc = requirements(&g, s, rt, backward, L.e, r);
    if (rc) snprintf(buf + at, sizeof buf - at, "%d", rc);
    else snprintf(buf + at, sizeof buf - at, "0 %d %lld %lld %lld %lld %zu %zu", r.mask, r.need_bytes[0], r.need_bytes[1], r.need_bytes[2],
                  r.need_bytes[3], r.ws, r.saved);
    return buf;
}

void table(int fin, int fout, int combin, int bf16, bool routes) {
    Shape s;
    if (!make_shape(s, fin, fout, combin, bf16)) { printf("%d %d %d %d : shape refused\n", fin, fout, combin, bf16); return; }
    for (const ListCase& L : LISTS) {
        if (combin && L.n > 41000) continue;  // (a combining layer never takes the row kernels: the large levels add nothing)
        for (int backward = 0; backward < 2; ++backward)
            for (int pieces = 0; pieces < 3; ++pieces)
                for (int aligned = 1; aligned >= (combin ? 1 : 0); --aligned) {  // (the pointer only matters to depth-wise rows)
                    printf("%d %d %d %d | %d %d %d | b%d p%d a%d :", fin, fout, combin, bf16, L.n, L.m, L.e, backward, pieces, aligned);
                    std::vector<std::string> seen;
                    char which[9] = {0};
                    for (int flags = 0; flags < 8; ++flags) {
                        const std::string v = sizes(L, s, backward, pieces, aligned != 0, flags, routes);
                        size_t k = std::find(seen.begin(), seen.end(), v) - seen.begin();
                        if (k == seen.size()) seen.push_back(v);
                        which[flags] = char('0' + k);
                    }
                    printf(" %s", which);
                    for (size_t k = 0; k < seen.size(); ++k) printf(" %s %s", k ? ";" : ":", seen[k].c_str());
                    printf("\n");
                }
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool routes = argc > 1 && std::string(argv[1]) == "--routes";
    for (const auto& c : COMBIN) table(c[0], c[1], 1, 0, routes);
    for (int f : DEPTHWISE) table(f, f, 0, 0, routes);
    for (int f : DEPTHWISE) table(f, f, 0, 1, routes);
    return 0;
}
