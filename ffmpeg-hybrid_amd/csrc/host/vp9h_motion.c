// vp9hip_motion_host: the motion field of one packet on the host, the C statement of the
// definition in include/vp9hip.h ("motion export"). k_motion (vp9hip_motion.hip) computes the
// same cells from the batch's resident blocks; this is what the tests compare it with and what
// the sanitizer builds run (tests/c/motion_host_check.c).
#include <string.h>

#include "../../../include/vp9hip.h"

// width / height of a block size in 4-pixel units; sizes below 8x8 cover their 8x8 unit
static const uint8_t bs_w4[VP9H_N_BS] = { 16, 16, 8, 8, 8, 4, 4, 4, 2, 2, 2, 2, 2 };
static const uint8_t bs_h4[VP9H_N_BS] = { 16, 8, 16, 8, 4, 8, 4, 2, 4, 2, 2, 2, 2 };

int vp9hip_motion_host(const vp9h_frame *pkt, int16_t *mv, uint8_t *info)
{
    if (!pkt || !mv || !info || pkt->width <= 0 || pkt->height <= 0 || (pkt->nblocks && !pkt->blocks))
        return VP9HIP_EINVAL;
    const int cols8 = (pkt->width + 7) >> 3, rows8 = (pkt->height + 7) >> 3;
    const int gw = 2 * cols8, gh = 2 * rows8;
    int written = 0;
    for (uint32_t n = 0; n < pkt->nblocks; n++) {
        const vp9h_block *b = &pkt->blocks[n];
        if (b->bs >= VP9H_N_BS || b->row >= rows8 || b->col >= cols8) continue;
        const int r0 = 2 * b->row, c0 = 2 * b->col;
        const int r1 = r0 + bs_h4[b->bs] < gh ? r0 + bs_h4[b->bs] : gh;
        const int c1 = c0 + bs_w4[b->bs] < gw ? c0 + bs_w4[b->bs] : gw;
        const uint8_t i0 = b->intra ? 255 : b->ref[0];
        const uint8_t i1 = (!b->intra && b->comp) ? b->ref[1] : 255;
        const uint8_t i3 = (uint8_t) (b->bs | b->skip << 4 | b->seg_id << 5);
        for (int r = r0; r < r1; r++)
            for (int c = c0; c < c1; c++) {
                const int i = (r & 1) * 2 + (c & 1);
                const size_t cell = (size_t) r * gw + c;
                uint8_t *q = info + cell * 4;
                int16_t *m = mv + cell * 4;
                q[0] = i0; q[1] = i1; q[2] = b->mode[i]; q[3] = i3;
                m[0] = i0 != 255 ? b->mv[i][0][0] : 0;
                m[1] = i0 != 255 ? b->mv[i][0][1] : 0;
                m[2] = i1 != 255 ? b->mv[i][1][0] : 0;
                m[3] = i1 != 255 ? b->mv[i][1][1] : 0;
                written++;
            }
    }
    return written;
}
