// Library-wide host utilities: thread-local error text, device selection, version.
#include <math.h>

#include <cstdarg>
#include <cstdio>

#include "common.hpp"
#include "grid.hpp"

namespace yta {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("no HIP device available (%s)", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return YTA_ERR_HIP;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (%d devices)", device, n);
        return YTA_ERR_INVALID;
    }
    YTA_HIP(hipSetDevice(device));
    return YTA_OK;
}

hipError_t host_wait(hipStream_t s) {
    constexpr int MAX_DEV = 64;
    thread_local hipEvent_t ev[MAX_DEV] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (s) {
        hipDevice_t sd;
        if (hipStreamGetDevice(s, &sd) == hipSuccess) dev = (int)sd;
    }
    if (dev < 0 || dev >= MAX_DEV) return hipStreamSynchronize(s);
    if (!ev[dev]) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        e = hipEventCreateWithFlags(&ev[dev], hipEventBlockingSync | hipEventDisableTiming);
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) {
            ev[dev] = nullptr;
            return hipStreamSynchronize(s);
        }
    }
    e = hipEventRecord(ev[dev], s);
    if (e != hipSuccess) return e;
    return hipEventSynchronize(ev[dev]);
}

}  // namespace yta

extern "C" {

int yta_version(void) { return 1; }

const char *yta_last_error(void) { return yta::g_err; }

int yta_device_count(int *count) {
    YTA_CHECK(count, YTA_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = e == hipSuccess ? n : 0;
    return YTA_OK;
}

int yta_apply_block_map(int gx, int n_streams, int *stream, int *block) {
    YTA_CHECK(gx > 0 && n_streams > 0 && stream && block, YTA_ERR_INVALID, "bad block map shape");
    for (int lin = 0; lin < gx * n_streams; ++lin)
        yta::xcd_stream_blocks(lin, gx, n_streams, stream[lin], block[lin]);
    return YTA_OK;
}

int yta_s1_pretest(int nr, const double *pool, int nc, const double *high, const double *score,
                   double thresh, unsigned char *out) {
    using namespace yta;
    YTA_CHECK(nr >= 0 && nc >= 0 && nc <= 65536 && (pool || !nr) && (high || !nc) &&
                  (score || !nc) && (out || !nr || !nc),
              YTA_ERR_INVALID, "bad pre-test shape");
    auto box = [](const double *p, int i) {
        return Box{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]};
    };
    // grid_build's header: the reduction over the usable boxes, then the binned boxes' largest
    // width and height (a sequential sum here: the mean may differ from the kernel's in its last
    // bits, which moves the scale by as much and no argument by anything)
    double v[6] = {0.0, 0.0, INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < nc; ++j) {
        const Box b = box(high, j);
        if (!box_usable(b)) continue;
        v[0] += fmax(b.x2 - b.x1, b.y2 - b.y1);
        v[1] += 1.0;
        v[2] = fmin(v[2], b.x1);
        v[3] = fmin(v[3], b.y1);
        v[4] = fmax(v[4], b.x1);
        v[5] = fmax(v[5], b.y1);
    }
    const double bthr = 4.0 * grid_mean_size(v);
    GridHdr h = grid_geometry(v, nc);
    for (int j = 0; j < nc; ++j) {
        const Box b = box(high, j);
        if (!grid_binned(b, bthr)) continue;
        h.maxw = fmax(h.maxw, b.x2 - b.x1);
        h.maxh = fmax(h.maxh, b.y2 - b.y1);
    }
    const double sc = grid_pack_scale(h);
    (void)score;    // read by the second stage only, which the kernel does not have
    (void)thresh;
    for (int i = 0; i < nr; ++i) {
        const uint2 a = box_pack16(box(pool, i), h.ox, h.oy, sc);
        for (int j = 0; j < nc; ++j) {
            const Box b = box(high, j);
            unsigned char r = 3;   // not binned: the kernel tests these pairs in float64 only
            if (grid_binned(b, bthr)) {
                const uint2 c = box_pack16(b, h.ox, h.oy, sc);
                r = box16_meet(a, c) ? 3 : 0;
            }
            out[(size_t)i * nc + j] = r;
        }
    }
    return YTA_OK;
}

}  // extern "C"
