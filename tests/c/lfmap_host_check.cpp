// lf_sb's chunk map (csrc/vp9hip_lfmap.h) on the CPU: a stand-alone program (its own main, no
// device, no Python). For the four chroma geometries at both pixel sizes, with the workgroup size
// the kernels use (128 threads for 4:2:0, 192 otherwise), it checks that the map
//   - enumerates every (plane, row, chunk) of the LF tile exactly once over (lane, u), and reports
//     "past the last chunk" for exactly the other NT * NU - NCHUNK slots;
//   - stays inside the LDS tile: every chunk's 16 bytes lie inside its row's pitch and its plane's
//     rows, and no two chunks overlap;
//   - equals the former per-chunk decode (two divisions of the chunk number) slot for slot, so in
//     particular gives the same set;
//   - keeps NU = ceil(NCHUNK / NT) chunks per thread.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../../ffmpeg-hybrid_amd/csrc/vp9hip_lfmap.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the per-chunk decode lf_sb used before: chunk number -> (plane, tile row, chunk column)
static void ref_chunk(int ci, int NY, int YK, int CR, int CK, int &p, int &r, int &k)
{
    if (ci < NY) { p = 0; r = ci / YK; k = ci - r * YK; }
    else { const int c = ci - NY; p = 1 + (c >= CR * CK); const int cc = c - (p - 1) * CR * CK; r = cc / CK; k = cc - r * CK; }
}

template <int PS, int SH, int SV> static void check()
{
    constexpr int NT = (SH && SV) ? 128 : 192;
    typedef LfMap<PS, SH, SV, NT> M;
    const char *name = PS == 1 ? "8-bit" : "16-bit";
    // the geometry, restated from its definition (vp9hip_kernels.hip, LfP)
    CHECK(M::CPX * PS == 16 && M::XL == M::CPX, "%s %d%d: chunk size", name, SH, SV);
    CHECK(M::YK * M::CPX == 64 + M::XL && M::CK * M::CPX == M::CW + M::XL, "%s %d%d: chunks per row", name, SH, SV);
    CHECK(M::NCHUNK == 72 * M::YK + 2 * (M::CH + 8) * M::CK, "%s %d%d: NCHUNK", name, SH, SV);
    CHECK(M::NU == (M::NCHUNK + NT - 1) / NT, "%s %d%d: NU", name, SH, SV);
    CHECK((M::YP * PS) % 4 == 0 && (M::UVP * PS) % 4 == 0, "%s %d%d: rows dword-aligned", name, SH, SV);

    std::set<std::tuple<int, int, int>> seen;
    std::vector<char> bytes[3];
    const int rows[3] = { 72, M::CR, M::CR }, pitch[3] = { M::YP, M::UVP, M::UVP }, width[3] = { 64 + M::XL, M::CW + M::XL, M::CW + M::XL };
    for (int p = 0; p < 3; p++) bytes[p].assign((size_t) rows[p] * pitch[p] * PS, 0);
    int past = 0;
    for (int lane = 0; lane < NT; lane++) {
        const typename M::Lane l = M::of(lane);
        for (int u = 0; u < M::NU; u++) {
            int p = -1, r = -1, k = -1;
            const int ci = lane + u * NT;
            const bool ok = M::chunk(l, u, p, r, k);
            CHECK(ok == (ci < M::NCHUNK), "%s %d%d lane %d u %d: valid %d", name, SH, SV, lane, u, (int) ok);
            if (!ok) { past++; continue; }
            int rp, rr, rk;
            ref_chunk(ci, M::NY, M::YK, M::CR, M::CK, rp, rr, rk);
            CHECK(p == rp && r == rr && k == rk, "%s %d%d lane %d u %d: (%d,%d,%d), the decode by division gives (%d,%d,%d)",
                  name, SH, SV, lane, u, p, r, k, rp, rr, rk);
            if (p < 0 || p > 2 || r < 0 || r >= rows[p] || k < 0 || (k + 1) * M::CPX > width[p]) {
                CHECK(false, "%s %d%d lane %d u %d: (%d,%d,%d) outside the tile", name, SH, SV, lane, u, p, r, k);
                continue;
            }
            CHECK(seen.insert(std::make_tuple(p, r, k)).second, "%s %d%d: (%d,%d,%d) twice", name, SH, SV, p, r, k);
            const int off = M::tile_off(p, r, k);
            CHECK(off == r * pitch[p] + k * M::CPX, "%s %d%d: tile_off(%d,%d,%d) = %d", name, SH, SV, p, r, k, off);
            CHECK(off >= 0 && (size_t) (off + M::CPX) * PS <= bytes[p].size() && off % pitch[p] + M::CPX <= pitch[p],
                  "%s %d%d: (%d,%d,%d) at %d leaves its LDS row", name, SH, SV, p, r, k, off);
            CHECK((off * PS) % 4 == 0, "%s %d%d: (%d,%d,%d) at %d not dword-aligned", name, SH, SV, p, r, k, off);
            if (off >= 0 && (size_t) (off + M::CPX) * PS <= bytes[p].size())
                for (int b = 0; b < 16; b++) {
                    CHECK(!bytes[p][(size_t) off * PS + b], "%s %d%d: (%d,%d,%d) overlaps another chunk", name, SH, SV, p, r, k);
                    bytes[p][(size_t) off * PS + b] = 1;
                }
        }
    }
    CHECK((int) seen.size() == M::NCHUNK, "%s %d%d: %d chunks of %d", name, SH, SV, (int) seen.size(), M::NCHUNK);
    CHECK(past == NT * M::NU - M::NCHUNK, "%s %d%d: %d slots past the end", name, SH, SV, past);
    for (int p = 0; p < 3; p++)
        for (int r = 0; r < rows[p]; r++)
            for (int k = 0; k * M::CPX < width[p]; k++)
                CHECK(seen.count(std::make_tuple(p, r, k)) == 1, "%s %d%d: (%d,%d,%d) missing", name, SH, SV, p, r, k);
    printf("%s ss %d%d: NT %d NU %d, %d chunks\n", name, SH, SV, NT, M::NU, M::NCHUNK);
}

int main()
{
    check<1, 1, 1>(); check<1, 1, 0>(); check<1, 0, 1>(); check<1, 0, 0>();
    check<2, 1, 1>(); check<2, 1, 0>(); check<2, 0, 1>(); check<2, 0, 0>();
    if (fails) { printf("lfmap_host_check: %d failures\n", fails); return 1; }
    printf("lfmap_host_check OK\n");
    return 0;
}
