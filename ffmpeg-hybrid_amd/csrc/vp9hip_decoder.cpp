// VP9 bitstream decoder over the C-ABI: the avcodec_send_packet / avcodec_receive_frame
// loop of libavcodec/vp9.c for AV_CODEC_ID_VP9, with the host parse (vp9h_stream) in
// front of the device pixel path (vp9hip_ctx).
//
// What it restates of the reference decode loop (vp9.c:1558-1865, vp9_decode_frame):
//   - superframes split into frames first (the vp9_superframe_split BSF the decoder
//     declares, vp9.c:1977; bsf/vp9_superframe_split.c:40-95);
//   - show_existing_frame outputs a reference slot without decoding (vp9.c:1636-1653);
//   - every decoded frame goes to the slots of its refresh mask (vp9.c:1686-1691,
//     1845-1849); hidden frames (show_frame = 0) are decoded but not output;
//   - inter frames read their LAST / GOLDEN / ALTREF slots (s->s.h.refidx).
//
// Pipeline:
//   1. host parse on a pool of threads. Frames of one parse chain parse in order on one
//      vp9h_stream; a keyframe starts a new chain on a fresh vp9h_stream, because its
//      parse depends on no earlier frame (vp9h_frame_type). All-keyframe streams thus
//      parse frame-parallel, GOP streams GOP-parallel (the reference's frame threads get
//      the same freedom from ff_thread_finish_setup after the header, vp9.c:1736);
//   2. in decode order, on the caller's thread: reference slots, device buffers, and
//      batches of up to max_batch frames staged and launched on the GPU
//      (vp9hip_stage_batch_refs: reference chains in order, independent chains
//      concurrently; the batch planning itself runs on host threads);
//   3. receive_frame hands out frames whose batch has been launched, in output order.
// Like libavcodec's frame threading this adds decoder delay (up to max_batch frames plus
// the frames in parse); flushing (send_packet with data = NULL) drains it.
// Errors are per frame (vp9hip_pipeline.h): a packet whose parse fails is reported by the
// send_packet / receive_frame call that consumes it and updates no reference slot (vp9.c
// fails that decode, :1827-1832, and refreshes no slot); a frame the device rejects, or
// one predicted from a failed frame, fails when it is received.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <utility>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/vp9hip.h"
#include "vp9hip_parse.h"
#include "vp9hip_pipeline.h"

using vp9hip::Chain;
using vp9hip::LFrame;
using vp9hip::ParseJob;
using vp9hip::ParsePool;

namespace {
struct Pending { vp9h_frame pkt; LFrame f; };   // f.refs: -1 for keyframes / intra-only
struct Out { int buf; int64_t pts; bool submitted; uint64_t id; int cs, full; };   // cs / full: the frame's colour space, range
// Batches are numbered as launched (1, 2, ...) and rotate over VP9HIP_PIPELINE_SLOTS batch
// slots (vp9hip::Ledger), so batches k + 1 and k + 2 are staged and planned while batch k's
// pixel kernels run. A frame's batch is the one that wrote its buffer (Ledger::seq_of). A
// batch is checked (vp9hip_sync_slot: its slot's work is drained, the planner's verdicts and
// k_lfr's hand-off timeout words are read) before its slot is staged again, which resets
// them, or before one of its frames is handed out, whichever comes first.
const int STALL = 1;                   // consume: no free device buffer until frames are released
}

struct vp9hip_decoder {
    vp9hip_decoder_params p;
    vp9hip_ctx *ctx = nullptr;
    bool configured = false, draining = false;
    bool stalled = false;                  // send_packet answered EAGAIN: receive must block
    bool started = false;                  // a packet was sent: the export flags are fixed
    int export_flags = 0;                  // vp9hip_decoder_set_export
    int cw = 0, ch = 0, cbpp = 0, css_h = 0, css_v = 0, nbufs = 0;
    int slot[8];
    std::vector<int> pins, busy, bw, bh;   // per device buffer
    vp9hip::Ledger led;                    // batches in flight, per-frame outcomes
    std::vector<Pending> batch;
    std::deque<Out> outq;
    // parse pipeline
    std::deque<std::unique_ptr<ParseJob>> inflight;   // decode order
    std::shared_ptr<Chain> chain;                     // the chain of the next non-key frame
    std::unique_ptr<ParsePool> pool;
    int max_inflight = 0;
};

static int slot_refs(const vp9hip_decoder *d, int b)
{
    int n = 0;
    for (int s = 0; s < 8; s++) n += d->slot[s] == b;
    return n;
}

static int alloc_buffer(vp9hip_decoder *d)
{
    for (int b = 0; b < d->nbufs; b++)
        if (!d->pins[b] && !d->busy[b] && !slot_refs(d, b)) return b;
    return -1;
}

// ---- parse (vp9hip_parse.h) ----
static void enqueue_parse(vp9hip_decoder *d, std::unique_ptr<ParseJob> j)
{
    ParseJob *raw = j.get();
    d->inflight.push_back(std::move(j));
    d->pool->enqueue(raw);
}

static bool front_done(vp9hip_decoder *d, bool block)
{
    if (d->inflight.empty()) return false;
    if (block) d->pool->wait(d->inflight.front().get());
    return d->pool->done(d->inflight.front().get());
}

static void wait_all_parsed(vp9hip_decoder *d)
{
    for (auto &j : d->inflight) d->pool->wait(j.get());
}

// ---- device side ----
// Stage + launch the pending frames as one batch in the next pipeline slot (frames the
// device rejects fail alone, Ledger::launch). 0, or a failure of the device context.
static int submit(vp9hip_decoder *d)
{
    if (d->batch.empty()) return 0;
    const int n = (int) d->batch.size();
    std::vector<const vp9h_frame *> pk(n);
    std::vector<LFrame> fr(n);
    for (int i = 0; i < n; i++) {
        pk[i] = &d->batch[i].pkt;
        fr[i] = d->batch[i].f;
    }
    const int ret = d->led.launch(d->ctx, pk, fr);
    for (auto &p : d->batch) {
        vp9h_frame_free(&p.pkt);
        d->busy[p.f.out]--;
        for (int r = 0; r < 3; r++)
            if (p.f.refs[r] >= 0) d->busy[p.f.refs[r]]--;
    }
    d->batch.clear();
    for (auto &o : d->outq) o.submitted = true;
    return ret < 0 ? ret : 0;
}

static int configure(vp9hip_decoder *d, const vp9h_frame &f)
{
    const int w = d->p.max_width > 0 ? d->p.max_width : f.width;
    const int h = d->p.max_height > 0 ? d->p.max_height : f.height;
    if (f.width > w || f.height > h) return VP9HIP_ENOSYS;
    // 8 reference slots, the batch being filled, the launched batches' frames still to be
    // received (VP9HIP_PIPELINE_SLOTS in flight), and the frames the caller holds
    const int nb = 8 + (VP9HIP_PIPELINE_SLOTS + 1) * d->p.max_batch + (d->p.extra_bufs > 0 ? d->p.extra_bufs : 4);
    int r = vp9hip_set_export(d->ctx, d->export_flags);   // the same flags again on a reconfigure
    if (r < 0) return r;
    r = vp9hip_configure(d->ctx, w, h, f.bpp, f.ss_h, f.ss_v, nb);
    if (r < 0) return r;
    d->configured = true;
    d->cw = w; d->ch = h; d->cbpp = f.bpp; d->css_h = f.ss_h; d->css_v = f.ss_v;
    d->nbufs = nb;
    d->pins.assign(nb, 0); d->busy.assign(nb, 0); d->bw.assign(nb, 0); d->bh.assign(nb, 0);
    d->led.reset_buffers(nb);
    for (int s = 0; s < 8; s++) d->slot[s] = -1;
    return 0;
}

// One parsed frame, in decode order: slots, buffer, batch. 0, STALL (no free buffer;
// the job stays queued) or an error.
static int consume_one(vp9hip_decoder *d, ParseJob &j)
{
    if (j.ret < 0) return j.ret;
    vp9h_frame &f = j.pkt;
    const vp9h_frame_info &info = j.info;
    if (info.show_existing_frame) {
        const int b = d->configured ? d->slot[info.show_slot & 7] : -1;
        if (b < 0) return VP9HIP_EINVALIDDATA;
        d->pins[b]++;
        d->outq.push_back({ b, j.pts, d->batch.empty(), d->led.holder(b), info.colorspace, info.full_range });
        return 0;
    }
    const bool intra = f.keyframe || f.intraonly;
    if (!d->configured || f.bpp != d->cbpp || f.ss_h != d->css_h || f.ss_v != d->css_v ||
        f.width > d->cw || f.height > d->ch) {
        // a new format or size: only at an intra frame with nothing outstanding
        int r = submit(d);
        if (r < 0) return r;
        bool idle = true;
        for (int b = 0; b < d->nbufs && idle; b++) idle = !d->pins[b];
        if (!intra) return d->configured ? VP9HIP_ENOSYS : VP9HIP_EINVALIDDATA;
        if (!idle) return STALL;          // frames of the old format are still out: receive / release them
        r = configure(d, f);
        if (r < 0) return r;
    }
    int out = alloc_buffer(d);
    if (out < 0) {                        // the batch's busy buffers come back when it is launched
        int r = submit(d);
        if (r < 0) return r;
        out = alloc_buffer(d);
        if (out < 0) return STALL;
    }
    int refs[3];
    for (int i = 0; i < 3; i++) {
        refs[i] = intra ? -1 : d->slot[info.ref_slot[i] & 7];
        if (!intra && refs[i] < 0) return VP9HIP_EINVALIDDATA;
    }
    Pending q;
    q.pkt = f;
    q.f = d->led.frame(out, refs);
    memset(&f, 0, sizeof(f));            // the batch owns the packet now
    d->busy[out]++;
    for (int i = 0; i < 3; i++)
        if (refs[i] >= 0) d->busy[refs[i]]++;
    d->bw[out] = q.pkt.width; d->bh[out] = q.pkt.height;
    for (int s = 0; s < 8; s++)
        if (info.refresh_mask & (1 << s)) d->slot[s] = out;
    d->batch.push_back(q);
    if (info.show_frame) {
        d->pins[out]++;
        d->outq.push_back({ out, j.pts, false, q.f.id, info.colorspace, info.full_range });
    }
    if ((int) d->batch.size() >= d->p.max_batch) return submit(d);
    return 0;
}

// Consume parsed frames in decode order; block: wait for their parse. Returns 0 when the
// parsed front is consumed (or nothing is ready), STALL, or an error.
static int consume(vp9hip_decoder *d, bool block, size_t keep = 0)
{
    while (d->inflight.size() > keep && front_done(d, block)) {
        int r = consume_one(d, *d->inflight.front());
        if (r == STALL) return STALL;
        d->inflight.pop_front();
        if (r < 0) return r;
    }
    return 0;
}

// ---- C-ABI ----
extern "C" void vp9hip_decoder_defaults(vp9hip_decoder_params *p)
{
    memset(p, 0, sizeof(*p));
    p->max_batch = 16;
    p->extra_bufs = 4;
    p->parse_threads = (int) std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
}

extern "C" int vp9hip_decoder_open(const vp9hip_decoder_params *params, vp9hip_decoder **out)
{
    if (!out) return VP9HIP_EINVAL;
    *out = nullptr;
    vp9hip_decoder *d = new vp9hip_decoder();
    if (params) d->p = *params; else vp9hip_decoder_defaults(&d->p);
    if (d->p.max_batch <= 0) d->p.max_batch = 1;
    if (d->p.max_batch > 256) d->p.max_batch = 256;
    if (d->p.parse_threads < 0) d->p.parse_threads = 0;
    if (d->p.parse_threads > 64) d->p.parse_threads = 64;
    // parse lookahead: enough frames that the pool keeps parsing while the caller's thread
    // waits on the device (the batches in flight)
    d->max_inflight = 4 * d->p.parse_threads + VP9HIP_PIPELINE_SLOTS * d->p.max_batch + 1;
    for (int s = 0; s < 8; s++) d->slot[s] = -1;
    int r = vp9hip_open(d->p.device, &d->ctx);
    if (r < 0) { vp9hip_decoder_close(d); return r; }
    vp9hip_set_timing(d->ctx, 0);             // every batch runs once: plain launches, no events
    vp9hip_set_graph(d->ctx, 0);
    d->pool.reset(new ParsePool(d->p.parse_threads));
    *out = d;
    return 0;
}

static void drop_inflight(vp9hip_decoder *d)
{
    wait_all_parsed(d);
    d->inflight.clear();
}

extern "C" void vp9hip_decoder_close(vp9hip_decoder *d)
{
    if (!d) return;
    if (d->pool) drop_inflight(d);
    d->pool.reset();
    for (auto &f : d->batch) vp9h_frame_free(&f.pkt);
    d->chain.reset();
    if (d->ctx) vp9hip_close(d->ctx);
    delete d;
}

extern "C" vp9hip_ctx *vp9hip_decoder_context(vp9hip_decoder *d) { return d ? d->ctx : nullptr; }

extern "C" int vp9hip_decoder_send_packet(vp9hip_decoder *d, const uint8_t *data, size_t size, int64_t pts)
{
    if (!d) return VP9HIP_EINVAL;
    if (!data || !size) {                      // flush: drain the decoder delay (receive_frame does it)
        d->draining = true;
        int r = consume(d, false);
        return r < 0 ? r : 0;
    }
    if (d->draining) return VP9HIP_EOF;
    d->started = true;
    size_t offs[8], sizes[8];
    const int nf = vp9h_superframe_split(data, size, offs, sizes, 8);
    if (nf < 0) return nf;
    // bound the frames in flight: consume parsed ones first; a stall (no free device
    // buffer) asks the caller to receive frames (avcodec_send_packet's EAGAIN). An earlier
    // frame's error found here is returned after this packet is queued: the packet is taken
    int err = 0;
    if (d->inflight.size() + nf > (size_t) d->max_inflight) {
        int r = consume(d, true, d->max_inflight > nf ? d->max_inflight - nf : 0);
        if (r == STALL) { d->stalled = true; return VP9HIP_EAGAIN; }
        if (r < 0) err = r;
    }
    d->stalled = false;
    for (int k = 0; k < nf; k++) {
        const int type = vp9h_frame_type(data + offs[k], sizes[k]);
        if (type < 0) return err < 0 ? err : type;
        std::unique_ptr<ParseJob> j(new ParseJob());
        j->data.assign(data + offs[k], data + offs[k] + sizes[k]);
        j->pts = pts;
        if (type == 0 || !d->chain) {          // a keyframe parses on a fresh stream
            int r = 0;
            std::shared_ptr<Chain> c = ParsePool::new_chain(&r);
            if (!c) return err < 0 ? err : r;
            d->chain = c;
        }
        j->chain = d->chain;
        enqueue_parse(d, std::move(j));
    }
    if (err < 0) return err;
    int r = consume(d, false);
    return r < 0 ? r : 0;
}

extern "C" int vp9hip_decoder_receive_frame(vp9hip_decoder *d, vp9hip_decoded_frame *out)
{
    if (!d || !out) return VP9HIP_EINVAL;
    int r = 0;
    if (d->outq.empty() || !d->outq.front().submitted) {   // nothing to hand out yet: make progress
        r = consume(d, d->draining);
        if (r < 0) return r;
    }
    if (d->draining) {                         // everything parsed that can be placed: launch it
        r = submit(d);
        if (r < 0) return r;
    }
    if (d->outq.empty())
        return d->draining && d->inflight.empty() && d->batch.empty() ? VP9HIP_EOF : VP9HIP_EAGAIN;
    if (!d->outq.front().submitted) return VP9HIP_EAGAIN;
    const Out o = d->outq.front();
    if (!d->led.error(o.id)) {                 // its batch may still run: drain and check it
        const uint64_t b = d->led.seq_of(o.buf);
        const int s = d->led.unchecked(b);
        if (s >= 0) {
            // the newest batch still running: EAGAIN (frame-threading delay), so the caller
            // sends the next packets while it runs; an older batch, a drain or a stalled
            // send_packet wait for it (and for the batches before it: checks run in order)
            if (!d->draining && !d->stalled && b == d->led.last() && vp9hip_slot_busy(d->ctx, s) == 1)
                return VP9HIP_EAGAIN;
            if ((r = d->led.check_through(d->ctx, b)) < 0) return r;
        }
    }
    d->outq.pop_front();
    if (const int e = d->led.error(o.id)) {    // rejected on the device, or read a failed frame
        d->pins[o.buf]--;
        return e;
    }
    memset(out, 0, sizeof(*out));
    out->buf = o.buf;
    out->width = d->bw[o.buf];
    out->height = d->bh[o.buf];
    out->bpp = d->cbpp;
    out->ss_h = d->css_h;
    out->ss_v = d->css_v;
    out->pts = o.pts;
    out->colorspace = o.cs;
    out->full_range = o.full;
    return 0;                      // the buffer stays pinned until vp9hip_decoder_release
}

extern "C" int vp9hip_decoder_release(vp9hip_decoder *d, int buf)
{
    if (!d || buf < 0 || buf >= d->nbufs || d->pins[buf] <= 0) return VP9HIP_EINVAL;
    d->pins[buf]--;
    return 0;
}

// Received frames to an output format (vp9hip_convert_frames, vp9hip_convert_frames_scaled
// when `scaled`, or vp9hip_convert_frames_resampled when `rs`, vp9hip_convert_frames_bicubic when `cubic` as well). They are complete (their batch was checked by receive_frame), so nothing is
// ordered here.
static int decoder_convert(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format, bool scaled,
                           int out_width, int out_height, void *dst_dev, int64_t pitch, int64_t frame_stride, void *stream,
                           const vp9hip_resample *rs = nullptr, bool cubic = false, const vp9hip_grade *grade = nullptr,
                           bool graded = false)
{
    if (!d || !frames || n <= 0 || !d->configured) return VP9HIP_EINVAL;
    std::vector<int> bufs(n);
    for (int i = 0; i < n; i++) {
        const vp9hip_decoded_frame &f = frames[i];
        if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
        if (f.width != frames[0].width || f.height != frames[0].height || f.colorspace != frames[0].colorspace ||
            f.full_range != frames[0].full_range) return VP9HIP_EINVAL;
        bufs[i] = f.buf;
    }
    vp9hip_out_desc o;
    memset(&o, 0, sizeof(o));
    o.format = format;
    const int cs = frames[0].colorspace;
    o.colorspace = cs == 0 || cs == 6 ? 2 : cs;    // unknown / reserved: BT.709
    o.full_range = frames[0].full_range;
    o.width = frames[0].width; o.height = frames[0].height;
    o.pitch = pitch; o.frame_stride = frame_stride;
    if (graded) return vp9hip_convert_frames_graded(d->ctx, bufs.data(), n, &o, rs, grade, dst_dev, stream);
    if (rs && cubic) return vp9hip_convert_frames_bicubic(d->ctx, bufs.data(), n, &o, rs, dst_dev, stream);
    if (rs) return vp9hip_convert_frames_resampled(d->ctx, bufs.data(), n, &o, rs, dst_dev, stream);
    if (scaled) return vp9hip_convert_frames_scaled(d->ctx, bufs.data(), n, &o, out_width, out_height, dst_dev, stream);
    return vp9hip_convert_frames(d->ctx, bufs.data(), n, &o, dst_dev, stream);
}

extern "C" int vp9hip_decoder_convert(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                                      void *dst_dev, int64_t pitch, int64_t frame_stride, void *stream)
{
    return decoder_convert(d, frames, n, format, false, 0, 0, dst_dev, pitch, frame_stride, stream);
}

extern "C" int vp9hip_decoder_convert_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                                             int out_width, int out_height, void *dst_dev, int64_t pitch,
                                             int64_t frame_stride, void *stream)
{
    return decoder_convert(d, frames, n, format, true, out_width, out_height, dst_dev, pitch, frame_stride, stream);
}

extern "C" int vp9hip_decoder_convert_resampled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                                                const vp9hip_resample *rs, void *dst_dev, int64_t pitch,
                                                int64_t frame_stride, void *stream)
{
    if (!rs) return VP9HIP_EINVAL;
    return decoder_convert(d, frames, n, format, false, 0, 0, dst_dev, pitch, frame_stride, stream, rs);
}

extern "C" int vp9hip_decoder_convert_bicubic(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                                              const vp9hip_resample *rs, void *dst_dev, int64_t pitch,
                                              int64_t frame_stride, void *stream)
{
    if (!rs) return VP9HIP_EINVAL;
    return decoder_convert(d, frames, n, format, false, 0, 0, dst_dev, pitch, frame_stride, stream, rs, true);
}

extern "C" int vp9hip_decoder_convert_graded(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                                             const vp9hip_resample *rs, const vp9hip_grade *grade, void *dst_dev,
                                             int64_t pitch, int64_t frame_stride, void *stream)
{
    if (!rs || !grade) return VP9HIP_EINVAL;
    return decoder_convert(d, frames, n, format, false, 0, 0, dst_dev, pitch, frame_stride, stream, rs, false, grade, true);
}

// The metrics of pairs of received frames (vp9hip_frame_metrics). The frames are complete and
// stay the caller's: nothing is ordered and nothing released here.
extern "C" int vp9hip_decoder_metrics(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                                      const vp9hip_decoded_frame *frames_b, int n, int64_t *out_dev, int32_t *cells_dev,
                                      void *stream)
{
    if (!d || !frames_a || n <= 0 || !d->configured) return VP9HIP_EINVAL;
    std::vector<int> ba(n), bb(frames_b ? n : 0);
    const vp9hip_decoded_frame &f0 = frames_a[0];
    for (int s = 0; s < (frames_b ? 2 : 1); s++)
        for (int i = 0; i < n; i++) {
            const vp9hip_decoded_frame &f = s ? frames_b[i] : frames_a[i];
            if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
            if (f.width != f0.width || f.height != f0.height || f.bpp != f0.bpp || f.ss_h != f0.ss_h || f.ss_v != f0.ss_v)
                return VP9HIP_EINVAL;
            (s ? bb : ba)[i] = f.buf;
        }
    return vp9hip_frame_metrics(d->ctx, ba.data(), frames_b ? bb.data() : nullptr, n, f0.width, f0.height, out_dev,
                                cells_dev, stream);
}

// The histograms of received frames (vp9hip_frame_histograms), under the metrics' rules: complete
// frames that stay the caller's, nothing ordered and nothing released; the size is the frames' own.
extern "C" int vp9hip_decoder_histograms(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                                         const vp9hip_hist_desc *desc, int32_t *out_dev, void *stream)
{
    if (!d || !frames || n <= 0 || !desc || !d->configured) return VP9HIP_EINVAL;
    std::vector<int> bufs(n);
    const vp9hip_decoded_frame &f0 = frames[0];
    const bool own = desc->colorspace < 0;
    for (int i = 0; i < n; i++) {
        const vp9hip_decoded_frame &f = frames[i];
        if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
        if (f.width != f0.width || f.height != f0.height || f.bpp != f0.bpp || f.ss_h != f0.ss_h || f.ss_v != f0.ss_v)
            return VP9HIP_EINVAL;
        if (own && (f.colorspace != f0.colorspace || f.full_range != f0.full_range)) return VP9HIP_EINVAL;
        bufs[i] = f.buf;
    }
    vp9hip_hist_desc o = *desc;
    o.width = f0.width; o.height = f0.height;
    if (own) {
        o.colorspace = f0.colorspace == 0 || f0.colorspace == 6 ? 2 : f0.colorspace;   // unknown / reserved: BT.709
        o.full_range = f0.full_range;
    }
    return vp9hip_frame_histograms(d->ctx, bufs.data(), n, &o, out_dev, stream);
}

// Motion export: the flags go to the context before it is configured (the first keyframe).
extern "C" int vp9hip_decoder_set_export(vp9hip_decoder *d, int flags)
{
    if (!d || d->started) return VP9HIP_EINVAL;
    const int r = vp9hip_set_export(d->ctx, flags);
    if (!r) d->export_flags = flags;
    return r;
}

// The field of a received frame: it is complete (receive_frame checked its batch) and stays
// until the buffer is released, so this only looks up. A show_existing_frame output holds the
// buffer of the frame it shows, and with it that frame's field.
extern "C" int vp9hip_decoder_frame_motion(vp9hip_decoder *d, const vp9hip_decoded_frame *f, void **mv, void **info,
                                           int *gw, int *gh, int64_t *pitch_cells)
{
    if (!d || !f || !d->configured || !(d->export_flags & VP9HIP_EXPORT_MOTION)) return VP9HIP_EINVAL;
    if (f->buf < 0 || f->buf >= d->nbufs || d->pins[f->buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
    return vp9hip_frame_motion(d->ctx, f->buf, mv, info, gw, gh, pitch_cells, nullptr);
}

extern "C" int vp9hip_decoder_frame_motion_acc(vp9hip_decoder *d, const vp9hip_decoded_frame *f, void **acc_dev,
                                               int *gw, int *gh, int64_t *pitch_cells, uint32_t *serial)
{
    if (!d || !f || !d->configured || !(d->export_flags & VP9HIP_EXPORT_MOTION_ACC)) return VP9HIP_EINVAL;
    if (f->buf < 0 || f->buf >= d->nbufs || d->pins[f->buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
    return vp9hip_frame_motion_acc(d->ctx, f->buf, acc_dev, gw, gh, pitch_cells, serial, nullptr);
}

extern "C" int vp9hip_decoder_frame_residual(vp9hip_decoder *d, const vp9hip_decoded_frame *f, void *planes[3],
                                             int64_t pitch[3])
{
    if (!d || !f || !d->configured || !(d->export_flags & VP9HIP_EXPORT_RESIDUAL)) return VP9HIP_EINVAL;
    if (f->buf < 0 || f->buf >= d->nbufs || d->pins[f->buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
    return vp9hip_frame_residual(d->ctx, f->buf, planes, pitch, nullptr, nullptr, nullptr);
}

// The residual tensors of received frames (vp9hip_residual_frames_scaled). The frames are
// complete and stay the caller's: nothing is ordered and nothing released here. A
// show_existing_frame output holds the buffer of the frame it shows, and with it that frame's field.
extern "C" int vp9hip_decoder_residual_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                                              const vp9hip_resid_desc *desc, void *dst_dev, void *stream)
{
    if (!d || !frames || n <= 0 || !desc || !d->configured || !(d->export_flags & VP9HIP_EXPORT_RESIDUAL)) return VP9HIP_EINVAL;
    std::vector<int> bufs(n);
    const vp9hip_decoded_frame &f0 = frames[0];
    const bool own = desc->colorspace < 0;
    for (int i = 0; i < n; i++) {
        const vp9hip_decoded_frame &f = frames[i];
        if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
        if (f.width != f0.width || f.height != f0.height || f.bpp != f0.bpp || f.ss_h != f0.ss_h || f.ss_v != f0.ss_v)
            return VP9HIP_EINVAL;
        if (own && (f.colorspace != f0.colorspace || f.full_range != f0.full_range)) return VP9HIP_EINVAL;
        bufs[i] = f.buf;
    }
    vp9hip_resid_desc o = *desc;
    if (own) {
        o.colorspace = f0.colorspace == 0 || f0.colorspace == 6 ? 2 : f0.colorspace;   // unknown / reserved: BT.709
        o.full_range = f0.full_range;
    }
    return vp9hip_residual_frames_scaled(d->ctx, bufs.data(), n, &o, dst_dev, stream);
}

// The motion tensors of received frames (vp9hip_motion_frames_scaled), under the same rules: the
// frames are complete and stay the caller's, the size is the frames' own, and a
// show_existing_frame output holds the shown buffer and with it that frame's fields. The runtime
// refuses VP9HIP_MVT_ACC on a context without the accumulated planes.
extern "C" int vp9hip_decoder_motion_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                                            const vp9hip_mvt_desc *desc, void *dst_dev, void *stream)
{
    if (!d || !frames || n <= 0 || !desc || !d->configured || !(d->export_flags & VP9HIP_EXPORT_MOTION)) return VP9HIP_EINVAL;
    std::vector<int> bufs(n);
    const vp9hip_decoded_frame &f0 = frames[0];
    for (int i = 0; i < n; i++) {
        const vp9hip_decoded_frame &f = frames[i];
        if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
        if (f.width != f0.width || f.height != f0.height) return VP9HIP_EINVAL;
        bufs[i] = f.buf;
    }
    vp9hip_mvt_desc o = *desc;
    o.width = f0.width; o.height = f0.height;
    return vp9hip_motion_frames_scaled(d->ctx, bufs.data(), n, &o, dst_dev, stream);
}

// The accumulated residual of pairs of received frames (vp9hip_acc_warp), under the metrics'
// rules: complete frames that stay the caller's, nothing ordered and nothing released. A
// show_existing_frame output names the shown buffer, so its field and serial are that frame's.
extern "C" int vp9hip_decoder_acc_warp(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                                       const vp9hip_decoded_frame *frames_b, int n, int mode, int output, void *dst_dev,
                                       uint8_t *mask_dev, void *stream)
{
    if (!d || !frames_a || !frames_b || n <= 0 || !d->configured) return VP9HIP_EINVAL;
    std::vector<int> ba(n), bb(n);
    const vp9hip_decoded_frame &f0 = frames_a[0];
    for (int s = 0; s < 2; s++)
        for (int i = 0; i < n; i++) {
            const vp9hip_decoded_frame &f = s ? frames_b[i] : frames_a[i];
            if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
            if (f.width != f0.width || f.height != f0.height || f.bpp != f0.bpp || f.ss_h != f0.ss_h || f.ss_v != f0.ss_v)
                return VP9HIP_EINVAL;
            (s ? bb : ba)[i] = f.buf;
        }
    return vp9hip_acc_warp(d->ctx, ba.data(), bb.data(), n, f0.width, f0.height, mode, output, dst_dev, mask_dev, stream);
}

// The accumulated residual at model size of pairs of received frames (vp9hip_acc_warp_scaled),
// under vp9hip_decoder_acc_warp's rules; the size is the frames' own, the colour description
// that of the frames a, which must share it, as vp9hip_decoder_residual_scaled takes it.
extern "C" int vp9hip_decoder_acc_warp_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                                              const vp9hip_decoded_frame *frames_b, int n, const vp9hip_warpt_desc *desc,
                                              void *dst_dev, void *stream)
{
    if (!d || !frames_a || !frames_b || n <= 0 || !desc || !d->configured) return VP9HIP_EINVAL;
    std::vector<int> ba(n), bb(n);
    const vp9hip_decoded_frame &f0 = frames_a[0];
    for (int s = 0; s < 2; s++)
        for (int i = 0; i < n; i++) {
            const vp9hip_decoded_frame &f = s ? frames_b[i] : frames_a[i];
            if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
            if (f.width != f0.width || f.height != f0.height || f.bpp != f0.bpp || f.ss_h != f0.ss_h || f.ss_v != f0.ss_v)
                return VP9HIP_EINVAL;
            if (!s && (f.colorspace != f0.colorspace || f.full_range != f0.full_range)) return VP9HIP_EINVAL;
            (s ? bb : ba)[i] = f.buf;
        }
    vp9hip_warpt_desc o = *desc;
    o.width = f0.width; o.height = f0.height;
    o.colorspace = f0.colorspace == 0 || f0.colorspace == 6 ? 2 : f0.colorspace;   // unknown / reserved: BT.709
    o.full_range = f0.full_range;
    return vp9hip_acc_warp_scaled(d->ctx, ba.data(), bb.data(), n, &o, dst_dev, stream);
}

// The accumulated propagation of received frames (vp9hip_acc_propagate), under
// vp9hip_decoder_acc_warp's rules: complete frames of one size that stay the caller's, nothing
// ordered and nothing released. The roots are serials, so the key frame needs no pin. A
// show_existing_frame output names the shown buffer, so its field is that frame's.
extern "C" int vp9hip_decoder_acc_propagate(vp9hip_decoder *d, const vp9hip_decoded_frame *frames,
                                            const uint32_t *root_serials, const int *src_index, int n, int m,
                                            const vp9hip_prop_desc *desc, const void *src_dev, void *dst_dev,
                                            uint8_t *valid_dev, void *stream)
{
    if (!d || !frames || n <= 0 || !desc || !d->configured || !(d->export_flags & VP9HIP_EXPORT_MOTION_ACC)) return VP9HIP_EINVAL;
    std::vector<int> bufs(n);
    const vp9hip_decoded_frame &f0 = frames[0];
    for (int i = 0; i < n; i++) {
        const vp9hip_decoded_frame &f = frames[i];
        if (f.buf < 0 || f.buf >= d->nbufs || d->pins[f.buf] <= 0) return VP9HIP_EINVAL;   // not held by the caller
        if (f.width != f0.width || f.height != f0.height) return VP9HIP_EINVAL;
        bufs[i] = f.buf;
    }
    vp9hip_prop_desc o = *desc;
    o.width = f0.width; o.height = f0.height;
    return vp9hip_acc_propagate(d->ctx, bufs.data(), root_serials, src_index, n, m, &o, src_dev, dst_dev, valid_dev, stream);
}

// avcodec_flush_buffers (vp9.c:1865-1883): drop the decoder delay and the reference
// state; frames already handed out stay valid until released.
extern "C" int vp9hip_decoder_flush(vp9hip_decoder *d)
{
    if (!d) return VP9HIP_EINVAL;
    drop_inflight(d);
    d->chain.reset();
    for (auto &p : d->batch) {
        vp9h_frame_free(&p.pkt);
        d->busy[p.f.out]--;
        for (int r = 0; r < 3; r++)
            if (p.f.refs[r] >= 0) d->busy[p.f.refs[r]]--;
    }
    d->batch.clear();
    for (auto &o : d->outq) d->pins[o.buf]--;
    d->outq.clear();
    for (int s = 0; s < 8; s++) d->slot[s] = -1;
    d->draining = false;
    d->stalled = false;
    d->led.reset();                            // vp9hip_flush drops the batches in flight
    return d->ctx ? vp9hip_flush(d->ctx) : 0;
}
