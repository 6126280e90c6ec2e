// anakin_amd/csrc/detout.hip - FP32 DetectionOutput (the reference: saber/funcs/detection_output.h; decode_bbox_* in
// saber/funcs/impl/x86/detection_helper.cpp; get_max_score_index / jaccard_overlap / apply_nms_fast / nms_detect in
// saber/funcs/impl/detection_helper.cpp). The reference's GPU route decodes on the device and runs nms_detect on the HOST between two
// copies and a stream synchronisation; here the whole operator is two launches with a fixed-shape output, so it can be part of a captured
// pass.
//
// Launch 1, one workgroup per (image, class), detout_direct_f32 (form 0) or detout_mask_f32 (form 1):
//   select  every prior with score > conf_thresh (a NaN fails) becomes a 64-bit key (ordered score bits << 32) | ~index: descending key
//           order IS the reference's stable sort (score descending, index ascending; -0 and +0 are one score). Keys are gathered into LDS and
//           sorted DETOUT_SORT_CAP at a time by a bitonic network, the first nms_top_k of every sort staying in front as the running top:
//           the top-K of a union is the top-K of the parts' top-Ks, so this is exact for any P. The gather's LDS counter hands out slots in
//           no fixed order; the keys are distinct, so the sorted sequence does not depend on it.
//   decode  only the <= nms_top_k survivors, into LDS, in the reference's float32 steps (no fma: the library is built with
//           -ffp-contract=off); CENTER_SIZE's exp is the double exponential rounded to float once, which is what expf gives.
//   nms     form 0: the candidates one after the other, the lanes testing the current one against the kept list in parallel, one workgroup
//           vote per candidate; the adaptive threshold (eta) is followed. form 1 (eta == 1): the whole "j is suppressed by i" relation of
//           the survivors as an m x m/64 bit matrix in LDS, every (i, j) with the same float32 expression, then ONE wave walks the rows and
//           ORs the masks - one barrier instead of one per candidate. Both keep exactly the candidates apply_nms_fast keeps, in its order.
//   The kept (score bits, index, box) of the (image, class) go to the op's scratch in that order.
// Launch 2, detout_pack_f32, one workgroup per image: the image's total; where it exceeds keep_top_k the keep_top_k-th largest key
//   (ordered score << 32) | ~(class * nms_top_k + position) by the same LDS selection - score descending, label ascending, index ascending,
//   which is what the reference's stable sort over its label-ascending list amounts to; the selected entries of a class are a prefix of its
//   list, found by a binary search. Every workgroup sums the counts of the images in front of it itself (N * C integers), so rows are
//   written straight to their final place: no atomics, no workgroup waits for another. Rows behind the total are written as -1 by the
//   same launch, image n taking every N-th.
// Every output row has one writer and one value: the forms are bit-identical.
#include "kernels.h"

#include <atomic>

namespace saber_mi355x {

namespace {

constexpr int TPB = 256;
constexpr int CAP = DETOUT_SORT_CAP;
constexpr int STEP = 4 * TPB;      // items examined between two looks at the fill
static_assert(STEP == 1024 && DETOUT_MAX_NMS_TOP_K + STEP <= CAP, "detout_keep_fits and the running top assume this");

__device__ __forceinline__ unsigned ordered_bits(float s) {      // monotone float -> unsigned; -0 counts as +0
    s = s + 0.f;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// bitonic sort of buf[0 .. n), n a power of two, descending; all TPB threads, buf complete and a barrier passed before the call
__device__ void sort_desc(unsigned long long* buf, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += TPB) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool desc = (i & k) == 0;
                const unsigned long long a = buf[i], b = buf[l];
                if ((a < b) == desc) { buf[i] = b; buf[l] = a; }
            }
            __syncthreads();
        }
}

// buf[0 .. topn) the running top, buf[topn .. topn + f) new keys: sorts them together, returns the new top's size
__device__ int flush_top(unsigned long long* buf, int topn, int f, int K) {
    if (f == 0) return topn;
    const int m = topn + f;
    int n2 = 2;
    while (n2 < m) n2 <<= 1;      // <= CAP: the caller never lets topn + f pass CAP
    for (int t = m + threadIdx.x; t < n2; t += TPB) buf[t] = 0ull;      // 0 is below every key
    __syncthreads();
    sort_desc(buf, n2);
    return m < K ? m : K;
}

// the K largest keys of key(0 .. total) in buf[0 .. return), descending; key returns 0 for "not a candidate". K <= CAP - STEP.
template <typename KeyFn>
__device__ int select_top(unsigned long long* buf, int* fill, long long total, int K, KeyFn key) {
    int topn = 0;
    if (threadIdx.x == 0) *fill = 0;
    __syncthreads();
    for (long long base = 0; base < total; base += STEP) {
        int f = *fill;
        __syncthreads();      // everyone has read the fill before anyone adds to it
        if (topn + f + STEP > CAP) {
            topn = flush_top(buf, topn, f, K);
            if (threadIdx.x == 0) *fill = 0;
            __syncthreads();
        }
        for (int u = 0; u < 4; ++u) {
            const long long item = base + u * TPB + threadIdx.x;
            if (item < total) {
                const unsigned long long k = key(item);
                if (k) buf[topn + atomicAdd(fill, 1)] = k;      // topn + fill < CAP: checked above
            }
        }
        __syncthreads();
    }
    const int f = *fill;
    __syncthreads();
    return flush_top(buf, topn, f, K);
}

struct Box { float x0, y0, x1, y1; };

__device__ __forceinline__ float box_size(const Box& b) {      // bbox_size, normalized
    if (b.x1 < b.x0 || b.y1 < b.y0) return 0.f;
    return (b.x1 - b.x0) * (b.y1 - b.y0);
}
// jaccard_overlap(bbox1 = a: the candidate, bbox2 = b: the box kept before it); std::max(p, q) = p < q ? q : p, std::min(p, q) = q < p ? q : p
__device__ __forceinline__ float overlap(const Box& a, const Box& b) {
    if (b.x0 > a.x1 || b.x1 < a.x0 || b.y0 > a.y1 || b.y1 < a.y0) return 0.f;
    const float ix0 = a.x0 < b.x0 ? b.x0 : a.x0, iy0 = a.y0 < b.y0 ? b.y0 : a.y0;
    const float ix1 = b.x1 < a.x1 ? b.x1 : a.x1, iy1 = b.y1 < a.y1 ? b.y1 : a.y1;
    const float inter = (ix1 - ix0) * (iy1 - iy0);
    return inter / (box_size(a) + box_size(b) - inter);
}

__device__ __forceinline__ float exp_f(float x) { return (float)exp((double)x); }

__device__ Box decode_box(const DetoutKArgs& a, int n, int i) {
    const float* l = a.loc + ((size_t)n * a.P + i) * 4;
    const float l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3];
    if (!a.prior) return Box{l0, l1, l2, l3};
    const float* p = a.prior + (size_t)i * 4;
    const float* v = p + (size_t)a.P * 4;
    const float p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
    if (a.code == 1) {      // CORNER
        if (a.vit) return Box{p0 + l0, p1 + l1, p2 + l2, p3 + l3};
        return Box{p0 + l0 * v[0], p1 + l1 * v[1], p2 + l2 * v[2], p3 + l3 * v[3]};
    }
    const float pw = p2 - p0, ph = p3 - p1;
    if (a.code == 3) {      // CORNER_SIZE
        if (a.vit) return Box{p0 + l0 * pw, p1 + l1 * ph, p2 + l2 * pw, p3 + l3 * ph};
        return Box{p0 + l0 * v[0] * pw, p1 + l1 * v[1] * ph, p2 + l2 * v[2] * pw, p3 + l3 * v[3] * ph};
    }
    const float pcx = (p0 + p2) / 2.f, pcy = (p1 + p3) / 2.f;      // CENTER_SIZE
    float cx, cy, w, h;
    if (a.vit) {
        cx = l0 * pw + pcx; cy = l1 * ph + pcy;
        w = exp_f(l2) * pw; h = exp_f(l3) * ph;
    } else {
        cx = v[0] * l0 * pw + pcx; cy = v[1] * l1 * ph + pcy;
        w = exp_f(v[2] * l2) * pw; h = exp_f(v[3] * l3) * ph;
    }
    return Box{cx - w / 2.f, cy - h / 2.f, cx + w / 2.f, cy + h / 2.f};
}

__device__ __forceinline__ float score_at(const DetoutKArgs& a, int n, int c, int i) {
    return a.prior ? a.conf[((size_t)n * a.P + i) * a.C + c] : a.conf[((size_t)n * a.C + c) * a.P + i];
}

// dynamic LDS: [region0: CAP keys; form 1 later reuses it for the bit matrix][K boxes][K prior indices][K kept positions][2 counters];
// the kernel declares no static LDS, so what the launcher asks for is all the workgroup holds
template <int FORM>
__global__ __launch_bounds__(TPB) void detout_nms_kernel(DetoutKArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    unsigned long long* buf = (unsigned long long*)dyn;
    Box* boxes = (Box*)(dyn + a.region0);
    int* idxs = (int*)(boxes + a.K);
    int* kp = idxs + a.K;
    int* s_fill = kp + a.K;
    int* s_kc = s_fill + 1;
    const int n = blockIdx.x / a.C, c = blockIdx.x % a.C, tid = threadIdx.x;
    if (c == a.bg) {      // (uniform) the background class keeps nothing
        if (tid == 0) a.cls_cnt[blockIdx.x] = 0;
        return;
    }
    const int m = select_top(buf, s_fill, a.P, a.K, [&](long long i) -> unsigned long long {
        const float s = score_at(a, n, c, (int)i);
        if (!(s > a.conf_t)) return 0ull;
        return ((unsigned long long)ordered_bits(s) << 32) | (unsigned)~(unsigned)i;
    });
    for (int t = tid; t < m; t += TPB) {
        const int i = (int)~(unsigned)buf[t];
        idxs[t] = i;
        boxes[t] = decode_box(a, n, i);
    }
    __syncthreads();      // buf is dead from here on
    int kc = 0;
    if (FORM == 0) {
        float thr = a.nms_t;
        for (int i = 0; i < m; ++i) {
            const Box bi = boxes[i];
            int bad = 0;
            for (int k = tid; k < kc; k += TPB)
                if (!(overlap(bi, boxes[kp[k]]) <= thr)) bad = 1;      // a NaN overlap suppresses
            if (!__syncthreads_or(bad)) {
                if (tid == 0) kp[kc] = i;
                ++kc;
                if (a.eta < 1.f && thr > 0.5f) thr *= a.eta;
                __syncthreads();
            }
        }
    } else {
        const int W = (m + 63) >> 6;
        unsigned long long* mask = buf;      // [m][W]: bit j of row i: j > i and candidate j does not pass against i
        for (int q = tid; q < m * W; q += TPB) {
            const int w = q / m, i = q - w * m;      // neighbouring lanes: neighbouring rows, the same 64 columns (LDS broadcast)
            unsigned long long bits = 0ull;
            if ((w << 6) + 63 > i) {
                const Box bi = boxes[i];
                for (int b = 0; b < 64; ++b) {
                    const int j = (w << 6) + b;
                    if (j > i && j < m && !(overlap(boxes[j], bi) <= a.nms_t)) bits |= 1ull << b;
                }
            }
            mask[(size_t)i * W + w] = bits;
        }
        __syncthreads();
        if (tid < 64) {      // one wave: lane l holds word l of the "suppressed" set (W <= 16)
            unsigned long long rem = 0ull;
            for (int w = 0; w < W; ++w) {
                const int left = m - (w << 6);
                const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
                unsigned lo = __shfl((unsigned)rem, w), hi = __shfl((unsigned)(rem >> 32), w);
                unsigned long long alive = ~(((unsigned long long)hi << 32) | lo) & valid;
                while (alive) {
                    const int b = __ffsll((long long)alive) - 1, i = (w << 6) + b;
                    if (tid == 0) kp[kc] = i;
                    ++kc;
                    if (tid < W) rem |= mask[(size_t)i * W + tid];
                    lo = __shfl((unsigned)rem, w); hi = __shfl((unsigned)(rem >> 32), w);
                    alive = ~(((unsigned long long)hi << 32) | lo) & valid & ~((2ull << b) - 1ull);
                }
            }
            if (tid == 0) *s_kc = kc;
        }
        __syncthreads();
        kc = *s_kc;
    }
    const size_t out = (size_t)blockIdx.x * a.K;
    for (int j = tid; j < kc; j += TPB) {
        const int t = kp[j], i = idxs[t];
        a.cls_key[out + j] = make_uint2(__float_as_uint(score_at(a, n, c, i)), (unsigned)i);
        const Box b = boxes[t];
        a.cls_box[out + j] = make_float4(b.x0, b.y0, b.x1, b.y1);
    }
    if (tid == 0) a.cls_cnt[blockIdx.x] = kc;
}

__device__ int block_sum(int v, int* red) {      // all TPB threads; red: TPB / 64 ints
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();      // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < TPB / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(TPB) void detout_pack_kernel(DetoutKArgs a) {
    __shared__ unsigned long long buf[CAP];
    __shared__ int s_fill, s_red[TPB / 64], s_scan[TPB], s_sel[TPB];
    const int n = blockIdx.x, tid = threadIdx.x;
    // the rows in front of this image, this image's total, the grand total: every workgroup sums the N * C counts itself
    int base = 0, total = 0, mine = 0;
    for (int i = 0; i < a.N; ++i) {
        int part = 0;
        for (int c = tid; c < a.C; c += TPB) part += a.cls_cnt[i * a.C + c];
        const int T = block_sum(part, s_red);
        const int kept = T < a.keep ? T : a.keep;
        if (i < n) base += kept;
        if (i == n) mine = T;
        total += kept;
    }
    const int* cnt = a.cls_cnt + (size_t)n * a.C;
    const uint2* keys = a.cls_key + (size_t)n * a.C * a.K;
    const float4* bxs = a.cls_box + (size_t)n * a.C * a.K;
    auto key_of = [&](int c, int j) -> unsigned long long {
        return ((unsigned long long)ordered_bits(__uint_as_float(keys[(size_t)c * a.K + j].x)) << 32) | (unsigned)~(unsigned)(c * a.K + j);
    };
    unsigned long long theta = 0ull;      // the smallest selected key; 0: everything is selected
    if (mine > a.keep) {      // (uniform) keep <= CAP - STEP here: saber_hip_detout_create refuses the rest
        (void)select_top(buf, &s_fill, (long long)a.C * a.K, a.keep, [&](long long f) -> unsigned long long {
            const int c = (int)(f / a.K), j = (int)(f - (long long)c * a.K);
            return j < cnt[c] ? key_of(c, j) : 0ull;
        });
        theta = buf[a.keep - 1];
    }
    int off = base;
    for (int c0 = 0; c0 < a.C; c0 += TPB) {
        const int c = c0 + tid;
        int sel = 0;
        if (c < a.C) {
            sel = cnt[c];
            if (theta) {      // the selected entries of a class are a prefix of its list: the first j whose key is below theta
                int lo = 0, hi = sel;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (key_of(c, mid) >= theta) lo = mid + 1; else hi = mid;
                }
                sel = lo;
            }
        }
        __syncthreads();
        s_sel[tid] = sel;
        s_scan[tid] = sel;
        __syncthreads();
        for (int o = 1; o < TPB; o <<= 1) {      // inclusive scan
            const int v = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const int nc = a.C - c0 < TPB ? a.C - c0 : TPB;
        for (int cc = 0; cc < nc; ++cc) {
            const int first = off + s_scan[cc] - s_sel[cc];
            for (int j = tid; j < s_sel[cc]; j += TPB) {
                const size_t e = (size_t)(c0 + cc) * a.K + j;
                float* r = a.y + (size_t)(first + j) * 7;      // first + j < base + min(mine, keep) <= N * keep
                const float4 b = bxs[e];
                r[0] = (float)n; r[1] = (float)(c0 + cc); r[2] = __uint_as_float(keys[e].x);
                r[3] = b.x; r[4] = b.y; r[5] = b.z; r[6] = b.w;
            }
        }
        off += s_scan[TPB - 1];
    }
    const long long rows = (long long)a.N * a.keep;
    for (long long q = tid;; q += TPB) {      // the rows behind the total: image n writes every N-th
        const long long r = total + n + (q / 7) * a.N;
        if (r >= rows) break;
        a.y[r * 7 + q % 7] = -1.f;
    }
    if (tid == 0) {
        a.count[1 + n] = mine < a.keep ? mine : a.keep;
        if (n == 0) a.count[0] = total;
    }
}

size_t region0_bytes(int form, int K) {
    size_t r = (size_t)CAP * 8;
    const size_t m = (size_t)K * ((K + 63) / 64) * 8;
    if (form == 1 && m > r) r = m;
    return (r + 15) & ~(size_t)15;
}

size_t lds_bytes(int form, int K) { return region0_bytes(form, K) + (size_t)K * (16 + 4 + 4) + 16; }

hipError_t detout_prepare() {
    static std::atomic<bool> done[64];      // per device, zero-initialised
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return e != hipSuccess ? e : hipErrorInvalidDevice;
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const void* fns[] = {(const void*)detout_nms_kernel<0>, (const void*)detout_nms_kernel<1>};
    for (const void* f : fns)
        if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(1, DETOUT_MAX_NMS_TOP_K))) != hipSuccess) return e;      // the most a launch asks for
    done[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

}  // namespace

size_t detout_lds_bytes(int form, int K) { return lds_bytes(form, K); }

hipError_t launch_detout_f32(int form, const DetoutKArgs& a0, hipStream_t s) {
    if (form < 0 || form > 1 || !a0.loc || !a0.conf || !a0.y || !a0.count || !a0.cls_cnt || !a0.cls_key || !a0.cls_box) return hipErrorInvalidValue;
    if (a0.N <= 0 || a0.C <= 0 || a0.P <= 0 || a0.K < 1 || a0.K > DETOUT_MAX_NMS_TOP_K || a0.keep < 1) return hipErrorInvalidValue;
    if ((long long)a0.N * a0.C >= (1ll << 31) || (long long)a0.C * a0.K >= (1ll << 31)) return hipErrorInvalidValue;
    if (!detout_keep_fits(a0.C, a0.K, a0.keep)) return hipErrorInvalidValue;      // the pack kernel's selection would not fit
    if (form == 1 && !(a0.eta == 1.f)) return hipErrorInvalidValue;
    const size_t lds = detout_lds_bytes(form, a0.K);
    if (lds > DETOUT_LDS_LIMIT) return hipErrorInvalidValue;
    hipError_t e = detout_prepare();
    if (e != hipSuccess) return e;
    DetoutKArgs a = a0;
    a.region0 = (int)region0_bytes(form, a0.K);
    const dim3 grid((unsigned)(a.N * a.C)), block(TPB);
    if (form == 0) hipLaunchKernelGGL(detout_nms_kernel<0>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(detout_nms_kernel<1>, grid, block, lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(detout_pack_kernel, dim3((unsigned)a.N), block, 0, s, a);
    return hipGetLastError();
}

}  // namespace saber_mi355x
