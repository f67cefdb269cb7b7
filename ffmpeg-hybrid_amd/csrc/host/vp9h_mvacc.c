// vp9hip_motion_acc_host: one frame of the accumulated-motion recurrence on the host, the C
// statement of the definition in include/vp9hip.h ("accumulated motion"). k_mvacc
// (vp9hip_mvacc.hip) walks the same chain inside a batch; this is what the tests compare it with
// and what the sanitizer builds run (tests/c/motion_acc_host_check.c, built without -fwrapv:
// the two sums are unsigned adds, so nothing here may overflow a signed integer).
#include <string.h>

#include "../../../include/vp9hip.h"

static int clampi(int v, int hi)
{
    return v < 0 ? 0 : v > hi ? hi : v;
}

// floor(v / 32) without shifting a negative value (what an arithmetic >> 5 gives)
static int floor32(int v)
{
    return v >= 0 ? v / 32 : -((31 - v) / 32);
}

int vp9hip_motion_acc_host(const int16_t *mv, const uint8_t *info, int gw, int gh, uint32_t serial,
                           const vp9hip_acc_cell *const parent[3], const int parent_end[3],
                           vp9hip_acc_cell *out)
{
    if (!mv || !info || !out || !parent || !parent_end || gw <= 0 || gh <= 0 || gw > 4096 || gh > 4096)
        return VP9HIP_EINVAL;
    for (int k = 0; k < 3; k++)
        if (!parent[k] && parent_end[k] != VP9HIP_ACC_END_NOFIELD && parent_end[k] != VP9HIP_ACC_END_SCALED)
            return VP9HIP_EINVAL;
    for (int r = 0; r < gh; r++)
        for (int c = 0; c < gw; c++) {
            const size_t cell = (size_t) r * gw + c;
            const uint8_t i0 = info[cell * 4];
            vp9hip_acc_cell o;
            memset(&o, 0, sizeof(o));
            if (i0 == 255) {
                o.root = serial;
                o.end = VP9HIP_ACC_END_INTRA;
                out[cell] = o;
                continue;
            }
            const int mx = mv[cell * 4], my = mv[cell * 4 + 1];
            if (i0 > 2 || !parent[i0]) {
                o.dx = mx; o.dy = my; o.hops = 1;
                o.end = (uint8_t) (i0 > 2 ? VP9HIP_ACC_END_NOFIELD : parent_end[i0]);
                out[cell] = o;
                continue;
            }
            const int pc = clampi(floor32(32 * c + 16 + mx), gw - 1);
            const int pr = clampi(floor32(32 * r + 16 + my), gh - 1);
            const vp9hip_acc_cell q = parent[i0][(size_t) pr * gw + pc];
            o.dx = (int32_t) ((uint32_t) mx + (uint32_t) q.dx);
            o.dy = (int32_t) ((uint32_t) my + (uint32_t) q.dy);
            o.root = q.root;
            o.hops = (uint16_t) (q.hops == 65535 ? 65535 : q.hops + 1);
            o.end = q.end;
            out[cell] = o;
        }
    return 0;
}
