// vp9h_webm_read_colour (csrc/host/vp9h_webm.c): a stand-alone program, no device, no Python,
// built plain and with ASan + UBSan. Files are written here, element by element, into exact-size
// heap blocks, so a read past `size` is a finding. Checked: a Colour element with every field
// (4- and 8-byte floats), a track without one, an element with only some fields, the file cut at
// every byte length (known-size and unknown-size Segment), and elements whose size runs past
// their parent.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

typedef struct { uint8_t b[1024]; size_t n; } Buf;

static void put_id(Buf *o, uint32_t id)
{
    int len = id > 0xFFFFFF ? 4 : id > 0xFFFF ? 3 : id > 0xFF ? 2 : 1;
    while (len--) o->b[o->n++] = (uint8_t) (id >> (8 * len));
}
// an element with a 2-byte size (or the 1-byte unknown size)
static void put_el(Buf *o, uint32_t id, const void *payload, size_t n, int unknown)
{
    put_id(o, id);
    if (unknown) o->b[o->n++] = 0xFF;
    else { o->b[o->n++] = (uint8_t) (0x40 | n >> 8); o->b[o->n++] = (uint8_t) n; }
    memcpy(o->b + o->n, payload, n);
    o->n += n;
}
static void put_uint(Buf *o, uint32_t id, uint32_t v)
{
    const uint8_t p[4] = { (uint8_t) (v >> 24), (uint8_t) (v >> 16), (uint8_t) (v >> 8), (uint8_t) v };
    put_el(o, id, p, 4, 0);
}
static void put_float(Buf *o, uint32_t id, double v, int bytes)
{
    uint8_t p[8];
    uint64_t u;
    if (bytes == 4) { const float f = (float) v; uint32_t w; memcpy(&w, &f, 4); u = w; }
    else memcpy(&u, &v, 8);
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t) (u >> (8 * (bytes - 1 - i)));
    put_el(o, id, p, (size_t) bytes, 0);
}

// fields: bit k set = field k of the Colour element is written; colour < 0: no element at all.
// *colour_size_at: where the Colour element's 2-byte size is in the file.
static void make_file(Buf *f, int fields, int float_bytes, int unknown_segment, size_t *colour_size_at)
{
    Buf col = { .n = 0 }, mm = { .n = 0 }, video = { .n = 0 }, te = { .n = 0 }, tracks = { .n = 0 }, seg = { .n = 0 },
        hdr = { .n = 0 }, info = { .n = 0 }, cl = { .n = 0 };
    static const uint32_t ids[7] = { 0x55B1, 0x55B2, 0x55B9, 0x55BA, 0x55BB, 0x55BC, 0x55BD };
    static const uint32_t vals[7] = { 9, 10, 1, 16, 9, 1000, 400 };
    for (int k = 0; k < 7; k++)
        if (fields >> k & 1) put_uint(&col, ids[k], vals[k]);
    if (fields >> 7 & 1) put_float(&mm, 0x55D9, 1000.0, float_bytes);
    if (fields >> 8 & 1) put_float(&mm, 0x55DA, 0.0625, float_bytes);
    if (mm.n) put_el(&col, 0x55D0, mm.b, mm.n, 0);
    put_uint(&video, 0xB0, 64);
    put_uint(&video, 0xBA, 48);
    size_t col_in_video = 0;
    if (fields >= 0) { col_in_video = video.n + 2; put_el(&video, 0x55B0, col.b, col.n, 0); }
    put_uint(&te, 0xD7, 1);
    put_uint(&te, 0x83, 1);
    put_el(&te, 0x86, "V_VP9", 5, 0);
    const size_t video_in_te = te.n + 1 + 2;
    put_el(&te, 0xE0, video.b, video.n, 0);
    put_el(&tracks, 0xAE, te.b, te.n, 0);
    put_uint(&info, 0x2AD7B1, 1000000);
    put_el(&seg, 0x1549A966, info.b, info.n, 0);
    const size_t te_in_seg = seg.n + 4 + 2 + 1 + 2;
    put_el(&seg, 0x1654AE6B, tracks.b, tracks.n, 0);
    put_uint(&cl, 0xE7, 0);
    put_el(&seg, 0x1F43B675, cl.b, cl.n, 0);
    put_el(&hdr, 0x4282, "webm", 4, 0);
    f->n = 0;
    put_el(f, 0x1A45DFA3, hdr.b, hdr.n, 0);
    const size_t seg_data = f->n + 4 + (unknown_segment ? 1 : 2);
    put_el(f, 0x18538067, seg.b, seg.n, unknown_segment);
    if (colour_size_at) *colour_size_at = seg_data + te_in_seg + video_in_te + col_in_video;
}

// the call on an exact-size copy of the first n bytes
static int read_cut(const Buf *f, size_t n, vp9h_webm_colour *c)
{
    uint8_t *p = malloc(n ? n : 1);
    if (!p) { printf("out of memory\n"); exit(2); }
    memcpy(p, f->b, n);
    const int r = vp9h_webm_read_colour(p, n, c);
    free(p);
    return r;
}

static int is_full(const vp9h_webm_colour *c)
{
    return c->present == 1 && c->matrix == 9 && c->bits_per_channel == 10 && c->range == 1 && c->transfer == 16 &&
           c->primaries == 9 && c->max_cll == 1000 && c->max_fall == 400 && c->luminance_max == 1000.0 &&
           c->luminance_min == 0.0625;
}
static int is_unspecified(const vp9h_webm_colour *c, int present)
{
    return c->present == present && c->matrix == 2 && c->transfer == 2 && c->primaries == 2 && !c->bits_per_channel &&
           !c->range && !c->max_cll && !c->max_fall && c->luminance_max == 0 && c->luminance_min == 0;
}

int main(void)
{
    Buf f;
    vp9h_webm_colour c;
    size_t at;
    for (int fb = 4; fb <= 8; fb += 4) {                   // every field, both float widths
        make_file(&f, 0x1FF, fb, 0, &at);
        CHECK(f.b[at - 2] == 0x55 && f.b[at - 1] == 0xB0);
        CHECK(read_cut(&f, f.n, &c) == 0 && is_full(&c));
        vp9h_webm_info info;
        vp9h_webm_cursor cur;
        CHECK(vp9h_webm_read_header(f.b, f.n, &info, &cur) == 0 && info.width == 64 && info.height == 48);
    }
    make_file(&f, -1, 8, 0, NULL);                         // no Colour element: not an error
    CHECK(read_cut(&f, f.n, &c) == 0 && is_unspecified(&c, 0));
    make_file(&f, 0, 8, 0, NULL);                          // an empty one
    CHECK(read_cut(&f, f.n, &c) == 0 && is_unspecified(&c, 1));
    make_file(&f, 1 << 3 | 1 << 7, 4, 0, NULL);            // transfer and LuminanceMax only
    CHECK(read_cut(&f, f.n, &c) == 0 && c.present && c.transfer == 16 && c.luminance_max == 1000.0 && c.matrix == 2 &&
          c.primaries == 2 && c.range == 0 && c.luminance_min == 0);
    CHECK(vp9h_webm_read_colour(NULL, 10, &c) == VP9HIP_EINVAL && vp9h_webm_read_colour(f.b, f.n, NULL) == VP9HIP_EINVAL);

    // the file cut at every length: an error, or the complete answer; nothing in between, and
    // (under ASan) no read past the cut
    for (int unknown = 0; unknown < 2; unknown++) {
        make_file(&f, 0x1FF, 8, unknown, &at);
        int ok = 0;
        for (size_t n = 0; n <= f.n; n++) {
            memset(&c, 0x5A, sizeof(c));
            const int r = read_cut(&f, n, &c);
            CHECK(r == VP9HIP_EINVALIDDATA || (r == 0 && is_full(&c)));
            ok += r == 0;
        }
        CHECK(ok >= 1);                                    // the whole file at least
        if (!unknown) CHECK(ok == 1);                      // a known-size Segment must be whole
    }
    // sizes that run past the parent: the Colour element's, and a field's inside it
    make_file(&f, 0x1FF, 8, 0, &at);
    const unsigned len = (unsigned) (f.b[at] & 0x3F) << 8 | f.b[at + 1];
    f.b[at + 1]++;                                         // one byte more than the Video element holds
    CHECK(read_cut(&f, f.n, &c) == VP9HIP_EINVALIDDATA);
    f.b[at] = 0x7F; f.b[at + 1] = 0xFE;                    // far past the file
    CHECK(read_cut(&f, f.n, &c) == VP9HIP_EINVALIDDATA);
    f.b[at] = (uint8_t) (0x40 | len >> 8); f.b[at + 1] = (uint8_t) len;
    CHECK(read_cut(&f, f.n, &c) == 0 && is_full(&c));
    f.b[at + 2 + 2] = 0x7F; f.b[at + 2 + 3] = 0xFE;        // the first field (2-byte ID, 2-byte size): past the element
    CHECK(read_cut(&f, f.n, &c) == VP9HIP_EINVALIDDATA);

    if (fails) { printf("webm_colour_check: %d failures\n", fails); return 1; }
    printf("webm_colour_check OK\n");
    return 0;
}
