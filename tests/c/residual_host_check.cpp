/* vp9hip_residual_host and the residual kernel's record guards (resid_rec_n,
 * csrc/vp9hip_residual.h) over packets that break their own counts: out-of-range blocks, eob
 * counts and coefficient totals that disagree, eob > N * N. The planes are exact-size heap blocks,
 * so ASan sees any access past them; guard bytes around a second copy catch a stray store in the
 * plain build. Every bad packet must return VP9HIP_EINVALIDDATA and leave the planes as they
 * were. A stand-alone program: no device, no Python
 * (make -C ffmpeg-hybrid_amd/csrc residual_host_check). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/vp9hip.h"
#include "../../ffmpeg-hybrid_amd/csrc/vp9hip_residual.h"

#define GUARD 64

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "residual_host_check: %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Packet {
    vp9h_frame f;
    std::vector<vp9h_block> blocks;
    std::vector<uint16_t> eobs;
    std::vector<int16_t> coefs;
    void bind()
    {
        // exact-size arrays: the vectors' heap blocks end where the data ends
        blocks.shrink_to_fit(); eobs.shrink_to_fit(); coefs.shrink_to_fit();
        f.blocks = blocks.data(); f.nblocks = (uint32_t) blocks.size();
        f.eobs = eobs.data(); f.neobs = (uint32_t) eobs.size();
        f.coefs = coefs.data(); f.ncoefs = coefs.size();
    }
};

static vp9h_block blk(int row, int col, int bs, int tx, int uvtx, int skip)
{
    vp9h_block b;
    memset(&b, 0, sizeof(b));
    b.row = (uint16_t) row; b.col = (uint16_t) col; b.bs = (uint8_t) bs; b.tx = (uint8_t) tx; b.uvtx = (uint8_t) uvtx;
    b.skip = (uint8_t) skip;
    for (int i = 0; i < 4; i++) b.mode[i] = 12;            /* ZEROMV */
    return b;
}

/* 66 x 34, 4:2:0: cols8 = 9, rows8 = 5; coded area 72 x 40 and 36 x 20. A good packet: one 64x64
 * block with 32x32 luma and 16x16 chroma transforms (the frame edge leaves 2 x 2 luma and 2 x 2
 * chroma tx blocks), one 8x8 block at column 8 with 4x4 transforms, the rest skipped. */
static Packet good()
{
    Packet p;
    memset(&p.f, 0, sizeof(p.f));
    p.f.width = 66; p.f.height = 34; p.f.bpp = 8; p.f.ss_h = p.f.ss_v = 1;
    p.blocks.push_back(blk(0, 0, VP9H_BS_64x64, 3, 2, 0));
    const int e64[12] = { 1024, 1, 0, 70, 256, 1, 0, 3, 0, 0, 256, 2 };   /* 4 luma, 4 + 4 chroma (ex = 16, ey = 10 >> 1 = 5 units) */
    for (int i = 0; i < 12; i++) p.eobs.push_back((uint16_t) e64[i]);
    p.blocks.push_back(blk(0, 8, VP9H_BS_8x8, 0, 0, 0));
    const int e8[6] = { 16, 1, 0, 5, 16, 0 };                             /* 2 x 2 luma, 1 + 1 chroma */
    for (int i = 0; i < 6; i++) p.eobs.push_back((uint16_t) e8[i]);
    for (int r = 1; r < 5; r++) p.blocks.push_back(blk(r, 8, VP9H_BS_8x8, 0, 0, 1));
    size_t nc = 0;
    for (uint16_t e : p.eobs) nc += e;
    for (size_t i = 0; i < nc; i++) p.coefs.push_back((int16_t) ((int) (i * 2654435761u >> 20) % 1201 - 600));
    p.bind();
    return p;
}

struct Planes {
    int16_t *pl[3];
    uint8_t *raw[3];
    ptrdiff_t pitch[3];
    int rows[3];
    size_t bytes[3];
    Planes(bool guarded)
    {
        const int cw[3] = { 72, 36, 36 }, ch[3] = { 40, 20, 20 };
        for (int p = 0; p < 3; p++) {
            pitch[p] = cw[p]; rows[p] = ch[p]; bytes[p] = (size_t) cw[p] * ch[p] * 2;
            raw[p] = (uint8_t *) malloc(bytes[p] + (guarded ? 2 * GUARD : 0));
            memset(raw[p], 0xa5, bytes[p] + (guarded ? 2 * GUARD : 0));
            pl[p] = (int16_t *) (raw[p] + (guarded ? GUARD : 0));
            memset(pl[p], 0x5a, bytes[p]);
        }
        g = guarded;
    }
    ~Planes() { for (int p = 0; p < 3; p++) free(raw[p]); }
    bool guards_ok() const
    {
        if (!g) return true;
        for (int p = 0; p < 3; p++)
            for (int i = 0; i < GUARD; i++)
                if (raw[p][i] != 0xa5 || raw[p][GUARD + bytes[p] + i] != 0xa5) return false;
        return true;
    }
    bool untouched() const
    {
        for (int p = 0; p < 3; p++)
            for (size_t i = 0; i < bytes[p]; i++)
                if (((const uint8_t *) pl[p])[i] != 0x5a) return false;
        return true;
    }
    bool g;
};

static int run(const Packet &p, Planes &P) { return vp9hip_residual_host(&p.f, P.pl, P.pitch, P.rows); }

/* a bad packet: the error code, nothing stored, in exact-size and in guarded planes */
static void expect_bad(Packet p, const char *what)
{
    p.bind();
    for (int g = 0; g < 2; g++) {
        Planes P(g != 0);
        const int r = run(p, P);
        if (r != VP9HIP_EINVALIDDATA || !P.untouched() || !P.guards_ok()) {
            fprintf(stderr, "residual_host_check: %s (%s planes): returned %d, planes %s, guards %s\n", what,
                    g ? "guarded" : "exact", r, P.untouched() ? "untouched" : "written", P.guards_ok() ? "whole" : "broken");
            fails++;
        }
    }
}

int main(void)
{
    {   /* the good packet: accepted, the same planes with and without guards, zeros where nothing is coded */
        const Packet p = good();
        Planes A(false), B(true);
        CHECK(run(p, A) == 0 && run(p, B) == 0 && B.guards_ok());
        for (int q = 0; q < 3; q++) CHECK(!memcmp(A.pl[q], B.pl[q], A.bytes[q]));
        bool any = false, in_range = true;
        for (int q = 0; q < 3; q++)
            for (size_t i = 0; i < A.bytes[q] / 2; i++) { any |= A.pl[q][i] != 0; in_range &= A.pl[q][i] >= -255 && A.pl[q][i] <= 255; }
        CHECK(any && in_range);
        for (int y = 8; y < 40; y++)                       /* the skipped 8x8 blocks below the coded one */
            for (int x = 64; x < 72; x++) CHECK(A.pl[0][y * 72 + x] == 0);
        for (int y = 32; y < 40; y++)                      /* luma tx block 2 of the 64x64 block has eob 0 */
            for (int x = 0; x < 32; x++) CHECK(A.pl[0][y * 72 + x] == 0);
    }
    {   /* out-of-range blocks and fields */
        Packet p = good(); p.blocks[1].row = 5; expect_bad(p, "row == rows8");
        p = good(); p.blocks[1].col = 9; expect_bad(p, "col == cols8");
        p = good(); p.blocks[0].row = 65535; p.blocks[0].col = 65535; expect_bad(p, "block far outside");
        p = good(); p.blocks[1].bs = VP9H_N_BS; expect_bad(p, "unknown block size");
        p = good(); p.blocks[1].bs = 255; expect_bad(p, "block size 255");
        p = good(); p.blocks[0].tx = 4; expect_bad(p, "tx size 4");
        p = good(); p.blocks[0].uvtx = 200; expect_bad(p, "uvtx 200");
        p = good(); p.blocks[1].intra = 1; p.blocks[1].mode[0] = 10; expect_bad(p, "intra mode 10");
        p = good(); p.f.lossless = 1; expect_bad(p, "lossless with 32x32 transforms");
    }
    {   /* counts that disagree */
        Packet p = good(); p.eobs.pop_back(); expect_bad(p, "one eob short");
        p = good(); p.eobs.push_back(0); expect_bad(p, "one eob more");
        p = good(); p.eobs.clear(); expect_bad(p, "no eobs");
        p = good(); p.coefs.pop_back(); expect_bad(p, "one coefficient short");
        p = good(); p.coefs.push_back(1); expect_bad(p, "one coefficient more");
        p = good(); p.coefs.resize(100); expect_bad(p, "coefficients end inside a block");
        p = good(); p.coefs.clear(); expect_bad(p, "no coefficients");
        p = good(); p.blocks[2].skip = 0; expect_bad(p, "a coded block without eobs");
    }
    {   /* eob > N * N (the totals kept consistent, so only that guard can refuse) */
        Packet p = good(); p.eobs[0] = 1025; p.coefs.push_back(1); expect_bad(p, "32x32 eob 1025");
        p = good(); p.eobs[4] = 257; p.coefs.push_back(1); expect_bad(p, "16x16 eob 257");
        p = good(); p.eobs[12] = 17; p.coefs.push_back(1); expect_bad(p, "4x4 eob 17");
        p = good(); p.eobs[13] = 2047; p.coefs.resize(p.coefs.size() + 2046, 1); expect_bad(p, "4x4 eob 2047");
        p = good(); p.eobs[2] = 65535; p.coefs.resize(p.coefs.size() + 65535, 1); expect_bad(p, "32x32 eob 65535");
    }
    {   /* the record guards the kernel shares: (key, eob, plane, ux0, uy0, sbx, sby, sb_cols, sb_rows, ss_h, ss_v, offset, total) */
        CHECK(resid_rec_n(12, 1024, 0, 8, 8, 0, 0, 2, 1, 1, 1, 0, 1024) == 32);
        CHECK(resid_rec_n(12, 1024, 0, 9, 8, 0, 0, 2, 1, 1, 1, 0, 1024) == 0);       /* reaches past the SB's right edge */
        CHECK(resid_rec_n(12, 1024, 0, 8, 9, 0, 0, 2, 1, 1, 1, 0, 1024) == 0);
        CHECK(resid_rec_n(12, 1, 1, 0, 0, 0, 0, 2, 1, 1, 1, 0, 1) == 32);            /* 32x32 chroma at 4:2:0: the whole square */
        CHECK(resid_rec_n(12, 1, 1, 1, 0, 0, 0, 2, 1, 1, 1, 0, 1) == 0);
        CHECK(resid_rec_n(12, 1, 1, 8, 0, 0, 0, 2, 1, 0, 0, 0, 1) == 32);            /* 4:4:4 */
        CHECK(resid_rec_n(12, 1, 2, 8, 8, 0, 0, 2, 1, 1, 0, 0, 1) == 0);             /* 4:2:2: 32 wide, 64 high */
        CHECK(resid_rec_n(12, 1, 2, 0, 8, 0, 0, 2, 1, 1, 0, 0, 1) == 32);
        CHECK(resid_rec_n(0, 16, 2, 7, 7, 1, 0, 2, 1, 1, 1, 0, 16) == 4);
        CHECK(resid_rec_n(0, 16, 2, 8, 7, 1, 0, 2, 1, 1, 1, 0, 16) == 0);
        CHECK(resid_rec_n(0, 16, 3, 0, 0, 0, 0, 2, 1, 1, 1, 0, 16) == 0);            /* plane 3 */
        CHECK(resid_rec_n(0, 17, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 100) == 0);           /* eob > N * N */
        CHECK(resid_rec_n(4, 65, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 100) == 0);
        CHECK(resid_rec_n(8, 257, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 1000) == 0);
        CHECK(resid_rec_n(12, 1025, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 5000) == 0);
        CHECK(resid_rec_n(16, 16, 0, 15, 15, 0, 0, 2, 1, 1, 1, 0, 16) == 4);         /* the WHT */
        CHECK(resid_rec_n(19, 16, 0, 15, 15, 0, 0, 2, 1, 1, 1, 0, 16) == 4);         /* its type bits do not matter */
        CHECK(resid_rec_n(16, 17, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 100) == 0);
        CHECK(resid_rec_n(13, 1, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 1) == 0);             /* a 32x32 type other than DCT_DCT */
        for (uint32_t key = 20; key < 32; key++) CHECK(resid_rec_n(key, 1, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 1) == 0);
        CHECK(resid_rec_n(0, 1, 0, 0, 0, 2, 0, 2, 1, 1, 1, 0, 1) == 0);              /* sbx == sb_cols */
        CHECK(resid_rec_n(0, 1, 0, 0, 0, 0, 1, 2, 1, 1, 1, 0, 1) == 0);              /* sby == sb_rows */
        CHECK(resid_rec_n(0, 1, 0, 0, 0, 0, 0, 2, 1, 2, 1, 0, 1) == 0);              /* no such subsampling */
        CHECK(resid_rec_n(0, 16, 0, 0, 0, 0, 0, 2, 1, 1, 1, 85, 100) == 0);          /* reads past the arena */
        CHECK(resid_rec_n(0, 16, 0, 0, 0, 0, 0, 2, 1, 1, 1, 84, 100) == 4);
        CHECK(resid_rec_n(0, 16, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0xfffffff8ull, 0xffffffffull) == 0);   /* no 32-bit wrap */
        CHECK(resid_rec_n(0, 1, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0xffffffffull + 5, 0xffffffffull) == 0);
    }
    {   /* bad arguments */
        const Packet p = good();
        Planes P(true);
        CHECK(vp9hip_residual_host(NULL, P.pl, P.pitch, P.rows) == VP9HIP_EINVAL);
        CHECK(vp9hip_residual_host(&p.f, NULL, P.pitch, P.rows) == VP9HIP_EINVAL);
        CHECK(vp9hip_residual_host(&p.f, P.pl, NULL, P.rows) == VP9HIP_EINVAL);
        CHECK(vp9hip_residual_host(&p.f, P.pl, P.pitch, NULL) == VP9HIP_EINVAL);
        int rows[3] = { 39, 20, 20 };
        CHECK(vp9hip_residual_host(&p.f, P.pl, P.pitch, rows) == VP9HIP_EINVAL);
        ptrdiff_t pitch[3] = { 72, 35, 36 };
        CHECK(vp9hip_residual_host(&p.f, P.pl, pitch, P.rows) == VP9HIP_EINVAL);
        vp9h_frame f = p.f;
        f.width = 0;
        CHECK(vp9hip_residual_host(&f, P.pl, P.pitch, P.rows) == VP9HIP_EINVAL);
        f = p.f; f.bpp = 9;
        CHECK(vp9hip_residual_host(&f, P.pl, P.pitch, P.rows) == VP9HIP_EINVAL);
        f = p.f; f.coefs = NULL;
        CHECK(vp9hip_residual_host(&f, P.pl, P.pitch, P.rows) == VP9HIP_EINVAL);
        CHECK(P.untouched() && P.guards_ok());
    }
    if (fails) { fprintf(stderr, "residual_host_check: %d checks failed\n", fails); return 1; }
    printf("residual_host_check OK\n");
    return 0;
}
