// anakin_amd/csrc/kernels.h — internal declarations shared by the HIP kernel TUs and the C-ABI TU.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// In-kernel phase stamps for scripts/probe/timeline_probe.hip (compiled with -DSABER_TIMELINE): every thread keeps the
// 100 MHz wall clock of each phase boundary in registers and thread 0 of every workgroup writes them out at the end
// (no memory traffic at the stamps themselves). Expands to nothing in the product build.
#ifdef SABER_TIMELINE
extern __device__ unsigned long long* saber_tl_buf;   // [blocks][16]
#define SABER_TL_DECL unsigned long long tl_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SABER_TL(i) tl_[i] = wall_clock64()
#define SABER_TL_FLUSH()                                                                   \
    do {                                                                                   \
        if (threadIdx.x == 0 && saber_tl_buf)                                              \
            for (int i_ = 0; i_ < 16; ++i_) saber_tl_buf[(size_t)blockIdx.x * 16 + i_] = tl_[i_]; \
    } while (0)
#else
#define SABER_TL_DECL do { } while (0)
#define SABER_TL(i) do { } while (0)
#define SABER_TL_FLUSH() do { } while (0)
#endif

namespace saber_mi355x {

enum { DT_F32 = 0, DT_S8 = 1, DT_U8 = 2 };

// Epilogue arithmetic selectors
enum {
    EPI_I8_CONV = 0,   // d=(float)acc; d+=bias; d*=scale; relu; [residual]; rne+saturate | f32
    EPI_I8_FC_S8 = 1,  // v=(float)acc*scale; v+=bias                (mkl_packed_int8_gemm.cpp:78-81)
    EPI_I8_FC_U8 = 2,  // acc+=bias_i (folded into comp); v = scale==1 ? (float)acc : scale*(float)acc
    EPI_F32 = 3,       // d=acc [+ prev]; d+=bias; relu
    EPI_I8_RAW_S32 = 4 // the exact int32 accumulator (+ comp), stored as int32 (INT8 GEMM, MklDnnGemm<s8|u8, s8, int>)
};
enum { RES_NONE = 0, RES_SUM_INPLACE = 1, RES_ELTWISE = 2 };

struct ConvKArgs {
    // ---- first 128 bytes (two 64-byte lines of the kernel-argument segment): everything the prologue needs to issue
    // its first global loads. hipcc fetches kernel arguments lazily with scalar loads, and every line touched before
    // the first operand load is an exposed scalar-cache miss (measured: loading all five lines of this block up front
    // costs +0.4 us per launch); keep the hot fields together and the rest behind them.
    const void* x;
    const void* w;      // repacked weights [K_pad][Kg_pad] (s8 or f32), zero padded
    const void* zero;   // >= 16 zero bytes in device memory (source of padded taps)
    int npx, nky;       // pixel tiles / out-channel tiles of the launch (1-D grid, XCD-aware tile order)
    unsigned mg_npx;    // ceil(2^32 / npx) when npx >= 2 and tiles * npx < 2^32, else 0: xcd_tile divides by __umulhi.
                        // Sits next to npx / nky on purpose: hipcc fetches it with the same wide scalar load (at the end of
                        // the block it cost a second, dependent scalar-load round trip: +0.2 us on every launch)
    int Kg_pad;         // reduction length padded to a multiple of the widest stage
    int M;              // N*OH*OW output pixels (GEMM columns)
    int OH, OW;
    float inv_ohw, inv_ow;  // 1/(OH*OW), 1/OW for the exact float-reciprocal div/mod
    int H, W, C;
    int stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int kh, kw;
    int steps;          // number of pipeline stages = ceil(Kg / elements-per-stage)
    int adv_c, adv_i, adv_j;   // per pipeline stage, the gather cursor advances by adv_c channels, adv_i / adv_j taps
                               // (stage elements = adv_c + C * (adv_i * kw + adv_j); set by the launcher)
    int in_u8;          // activations are u8: shift to s8 by XOR 0x80 (compensated through comp)
    int kw_pad;         // C4 mode: kw rounded up to 4
    // ---- the rest: epilogue and special-kernel parameters (fetched while the first loads are in flight) -----------
    void* y;
    const void* res;
    const float* bias;  // INT8 conv: pre-scaled bias_p; FC/F32: plain bias; may be null
    const float* scale; // per out-channel scale (INT8 paths)
    const int* comp;    // per out-channel int32 offset (u8 shift compensation [+ FC int bias]); may be null
    int N, K;
    int Kg;             // real reduction length in elements (kh*kw*C, or kh*kw_pad*4 in C4 mode)
    int Cin;            // stem kernel with fused quantisation: channels of the f32 NCHW image (<= 4)
    float qinv;         // ... and 1/in_scale
    int out_dtype;
    int out_nchw;       // f32 outputs only
    int relu;
    float neg_slope;    // FP32 convs with relu: negative inputs are multiplied by it (0: plain ReLU)
    int epi;
    int res_mode, res_relu, res_dtype;
    float sum_scale, coeff_conv, coeff_res, scale_conv, scale_res;
    // sibling pair (two convs over one input in one launch): rows [0,K1) -> y (stride K1, relu/out_dtype),
    // rows [K1, K1+K2) -> y2 (stride K2, relu2/out_dtype2); K = K1 + K2. K2 == 0: ordinary conv.
    void* y2;
    int K1, K2, relu2, out_dtype2;
    int pool_oh, pool_ow;   // fused 3x3 / stride-2 max pooling (conv_stem_pool_kernel): pooled output dims
    // RES_ELTWISE with a spatially subsampled residual: res is [N][res_H][res_W][K] and output pixel (n, oy, ox) adds
    // res[n][oy * res_sub][ox * res_sub] - a 1x1 / stride-s max pooling (one element per window: the identity on it)
    // folded into the read. res_sub <= 1: res is [M][K].
    int res_sub, res_H, res_W;
    int w_plane_chunks;     // MODE 3 (FP32 on three bf16 planes): 16-byte chunks between the weight planes (K_pad * Kg_pad / 8)
    // FP32 split-K (conv_igemm_impl.h): 2^ksplit_sh workgroups share one output tile, each reduces a slice of the stages; the
    // partial accumulators meet in `part` ([tile][split][wave][fragment][lane] v4f) and the LAST one to arrive on the tile's
    // counter sums them in split order (deterministic) and runs the epilogue. All splits of a tile run on ONE XCD (workgroups
    // 8 apart share an XCD), so the hand-off needs no L2 write-back: plain stores, s_waitcnt vmcnt(0), the counter, an L1
    // invalidate, plain loads - what profiles/r03/boundary_probe.txt measured.
    int ksplit_sh;          // log2 of the split count (0: ordinary launch)
    float* part;
    unsigned* part_ctr;     // [tiles], zero between launches
    unsigned* part_err;     // host-visible (pinned) word: a launch whose splits did NOT share an XCD counts itself here (the host
                            // turns that into an error status on the operator's next run and switches its split-K off); may be null
};

// conv3x3_img_kernel takes the common block plus its slab geometry (kept out of ConvKArgs: every byte of kernel
// argument is copied per launch by the eager path, measured +0.2 us per launch for +48 bytes)
struct ImgKArgs {
    ConvKArgs c;
    int ib, rb, nw, nrs;    // images / output rows per workgroup slab, waves per workgroup, row slabs per image
    unsigned mg[6];         // ceil(2^32 / d) for d = halo pixels per image, halo width, OW, rb*OW, tail_rows*OW, nrs
                            // (q = __umulhi(n, mg) == n / d for every n * d < 2^32, d >= 2: no integer division on device)
};
static_assert(offsetof(ConvKArgs, y) == 128, "hot kernel arguments fill exactly the first two 64-byte lines");

// conv_stem_pool_pair_kernel (conv_stem.h): the fused stem conv + max pooling with the sibling pair of 1x1 convs that reads the pooled
// tensor in the same launch. t.w: the pair's weights (first conv's rows, then the second's) in MFMA A-fragment order, per 32-channel
// group two fragments of 1 KB (row rho of fragment mf = channel base + (rho >> 2) * 8 + mf * 4 + (rho & 3)); t.prm: per 4 channels
// {scale[4], bias'[4], comp[4]}, padded to 256 x 16 bytes. c.y: the pooled tensor, or null when nothing else reads it.
struct StemPairTail {
    const void* w;
    const void* prm;
    void* y1;             // [pooled pixels][K1]
    void* y2;             // [pooled pixels][K2]
    int K1, K2;           // multiples of 32, K1 + K2 <= 320
    int relu1, relu2, u8_1, u8_2;
};
struct StemPairKArgs {
    ConvKArgs c;
    StemPairTail t;
};

// conv1x1_chain_kernel (conv1x1_chain.hip): a 1x1 conv with the fused eltwise epilogue (ResNet branch2c + sum + relu)
// followed by the next block's 1x1 branch2a conv on the same pixels, one launch.
constexpr int STAGE_MAX_TENSORS = 24;
struct ChainKArgs {
    const void* x;        // first conv's input [M][C1], s8 or u8
    const void* wstream;  // both convs' s8 weights in the order the four waves consume them (api.hip: pack_chain_stream)
    const void* res;      // residual [M][K1] s8
    const void* prm1;     // first conv: per 4 channels {scale[4], bias'[4], comp[4]} (48 bytes)
    const void* prm2;     // second conv, same layout (padded to a multiple of 64 x 16 bytes)
    void* y1;             // [M][K1] s8: the eltwise output (the next block's shortcut)
    void* y2;             // [M][K2] s8 / u8: the second conv's output
    int M, in_u8;
    int relu1, res_relu;
    float coeff_conv, scale_conv, coeff_res, scale_res;
    int relu2, out_u8_2;
    // with the block's 3x3 conv in front (conv1x1_chain_kernel<..., C3 = true>): x is ITS input [N][H][W][C1]
    const void* prm0;     // the 3x3 conv's {scale, bias', comp}, same layout
    const void* zero;     // >= 16 zero bytes (padding taps)
    int N, H, W;
    int tiles_x, tiles_per_img;        // 16-column tiles per row, tiles per image
    unsigned mg_tiles_x, mg_tpi;       // ceil(2^32 / d) for the two, 0 when d == 1
    int in0_u8, relu0;                 // the 3x3 conv's input dtype / relu (its output dtype is in_u8)
    int s0, H0, W0;                    // stride of the leading 3x3 conv (1 | 2) and, for 2, its input dims (H, W are the output's)
    int res_sub, res_H, res_W;         // s0 == 2: the shortcut is [N][res_H][res_W][K1], read at (y * res_sub, x * res_sub)
    // the second conv as a sibling pair (strided head + the next stage's branch1 / branch2a): rows >= k2_split -> y2b [M][K2 - k2_split]
    void* y2b;
    int k2_split, relu2b, out_u8_2b;
};
// cooperative form (conv_chain_coop.hip): TWO workgroups of one XCD per pixel tile, each computing half of every conv's output
// channels; the 3x3 conv's tile and the first 1x1 conv's tile are handed over through that XCD's L2. (Its own block: every byte of
// kernel argument is copied per launch by the eager path - the ordinary chain launches do not pay for these fields.)
struct CoopKArgs {
    ChainKArgs c;
    unsigned long long* coop_ctr;      // [tiles][2 barriers][16]: arrival counters, one per 128-byte line (parity protocol: never reset)
    void* coop_xch;                    // [tiles][16 pixels][C1] the 3x3 conv's 8-bit output tile
    unsigned* coop_xcc;                // [tiles][32]: words 0 / 1 = the XCD each half ran on (checked against each other); a line per tile
    unsigned* coop_err;                // host-visible word: placement violations / barrier time-outs are counted here
    int n_tiles;
};
bool conv1x1_chain_ok(int c1, int k1, int k2);
// rows: 16-pixel fragments per workgroup (with3x3: rows of its 16-column tile), waves per workgroup (4 | 8), split: workgroups the second
// conv's output channels are split over (1 | 2) - the decoded fields of a ChainForm (api_internal.h); k2 == 0: no second conv
hipError_t launch_conv1x1_chain(const ChainKArgs& a, int c1, int k1, int k2, int rows, int waves, int split, int with3x3, hipStream_t s);
// conv3x3 + conv1x1 (+ eltwise) + conv1x1 at C1 = 256 with the weight stream split over two cooperating workgroups per pixel tile
hipError_t launch_conv_chain_coop(const CoopKArgs& a, hipStream_t s);

// conv_stage4_c256_kernel (conv_stage_coop.hip): a RUN of res4 blocks (each: conv 3x3 -> conv 1x1 + eltwise -> next block's conv 1x1,
// C = 256) as one persistent launch, four cooperating workgroups per tile of 2 rows x 16 columns, all tiles of an image on one XCD
struct StageBlk {                      // one block's constants; a table of these in device memory, read with scalar loads
    const void* wstream;               // [quarter][wave] fragments (api_chain.hip: pack_coop4_stream)
    const void* prm0;                  // {scale, bias', comp} per 4 channels of the 3x3 / first 1x1 / second 1x1 conv (padded: ChainKArgs)
    const void* prm1;
    const void* prm2;
    float coeff_conv, scale_conv, coeff_res, scale_res;
    int in0_u8, relu0, in_u8, relu1, res_relu, relu2, out_u8_2, pad_;
};
template <int MAXB>                    // blocks per launch this argument block has room for (8: 192 bytes of output pointers, 24: 448)
struct Stage4KArgs {
    const void* x;                     // the first block's 3x3 input [N][H][W][256]
    const void* res;                   // the first block's shortcut [N][H][W][1024] s8
    const void* zero;                  // >= 16 zero bytes
    const StageBlk* blk;
    unsigned long long* grp_ctr;       // [tiles][32]: a tile's two hand-off counters (words 0 and 16), a 256-byte pair of lines per tile
    unsigned long long* img_ctr;       // [images][tiles per image + 1][16]: one 128-byte line per edge between two tile rows; words 0 / 1 = the counters of even / odd blocks
    void* xch;                         // [tiles][32 pixels][256]: the 3x3 conv's 8-bit output tile
    unsigned* xcc;                     // [tiles][32]: words 0..3 = the XCD each quarter ran on
    unsigned* err;                     // host-visible word: placement violations / barrier time-outs are counted here
    int nblk, N, H, W;
    int tiles_x, tiles_per_img;        // 16-column tiles per row pair, tiles per image
    unsigned mg_tiles_x, mg_tpi, mg_wpi;   // ceil(2^32 / d) for tiles_x, tiles_per_img, 4 * tiles_per_img; 0 when d == 1
    int per_image;                     // 1: workgroup b -> image (b / 8 / wpi) * 8 + b % 8 (required for nblk > 1); 0: tiles round-robin
    void* y1[MAXB];                    // per block [M][1024] s8: the eltwise output (the operator's own output tensor)
    void* y2[MAXB];                    // per block [M][256] s8 / u8: the second 1x1 conv's output = the next block's 3x3 input
    void* head_y;                      // with a head: the pair's second output [M][256] = the first block's 3x3 input (x is then the pair's input)
};
constexpr int STAGE4_SHORT = 8, STAGE4_LONG = 24;
// tail: behind the nblk blocks the strided head that follows the stage in ResNet (conv 3x3 / stride 2 -> conv 1x1 + eltwise, shortcut = the
// last block's y1 sub-sampled by 2) runs in the same launch: blk[nblk] = its constants (wstream: the 18 + 8 fragments of the first two convs
// per (quarter, wave); prm2 unused but readable), y1[nblk] = its output [N][ceil(H/2)][ceil(W/2)][1024] s8. Needs nblk >= 2, nblk + 1 <= MAXB.
// head: in FRONT of the blocks the sibling pair of 1x1 convs that feeds the first block (res4a_branch1: 512 -> 1024, s8 = the shortcut;
// res4a_branch2a: 512 -> 256 = the 3x3 input) runs in the same launch: x = the pair's input [N][H][W][512], res is not read and the shortcut
// tensor not written (it stays in LDS), head_y = the second conv's output, blk[-1] = the pair's constants (wstream: 16 + 4 fragments
// per (quarter, wave); prm1 / prm2 the two convs'; prm0 unused but readable; in_u8, relu1, relu2, out_u8_2). Needs an image per XCD.
hipError_t launch_conv_stage4(const Stage4KArgs<STAGE4_SHORT>& a, bool tail, bool head, hipStream_t s);
hipError_t launch_conv_stage4(const Stage4KArgs<STAGE4_LONG>& a, bool tail, bool head, hipStream_t s);
// the res3 stage (C = 128): one workgroup per tile, an image per XCD, nblk >= 2; grp_ctr / xch unused; tiles_x in {1, 2, 4}
hipError_t launch_conv_stage1_c128(const Stage4KArgs<STAGE4_SHORT>& a, hipStream_t s);
hipError_t launch_conv_stage1_c128(const Stage4KArgs<STAGE4_LONG>& a, hipStream_t s);
// the res2 stage (C = 64): the same kernel body with four waves, FOUR workgroups per CU (an image's tiles_per_img workgroups must all be
// resident on its XCD's 32 CUs: conv_stage1_c64_blocks_per_cu() * 32 >= tiles_per_img); a null y1[k] is not stored
hipError_t launch_conv_stage1_c64(const Stage4KArgs<STAGE4_SHORT>& a, hipStream_t s);
hipError_t launch_conv_stage1_c64(const Stage4KArgs<STAGE4_LONG>& a, hipStream_t s);
int conv_stage1_c64_blocks_per_cu();

// stage_xcd_kernel (stage_xcd.hip): a run of INT8 convolutions over small images as ONE persistent launch, one image per XCD
// at a time, the phases separated by an XCD-local barrier instead of a kernel boundary.
struct StagePhase {              // in device memory, read with scalar loads
    int type;                    // kernel variant: stage_xcd_type(tiles per CU, k-steps per wave, 3x3)
    int cin, cout;
    int in_t, out_t, res_t;      // tensor slots (StageKArgs::t)
    int in_u8, relu, out_u8;     // input dtype, the conv's own relu, output dtype of the plain epilogue
    int elt, res_relu;           // fused SaberEltwise epilogue (s8 residual, s8 output); relu after the sum
    float coeff_conv, scale_conv, coeff_res, scale_res;
    unsigned w_chunk, prm_chunk; // offsets in 16-byte chunks into StageKArgs::weights / prm
    int barrier;                 // an earlier phase of this launch wrote this phase's input / residual: XCD barrier first
    int reload;                  // bring the input image into LDS (0: the previous phase left it there)
    unsigned pch, mg_pch;        // LDS pixel pitch in chunks (cin / 16 + 1) and ceil(2^32 / pch)
    int red_chunk;               // LDS offset (chunks) of the cross-wave reduction buffer
    int pool_t;                  // >= 0: also write the global AVERAGE pooling of this phase's output, [n_img][cout] 8-bit of the output's
    float pool_idiv;             // dtype, to that slot: (float)(int32 sum over the pixels) * pool_idiv, rne, saturate (the INT8 pooling op)
};
static_assert(sizeof(StagePhase) == 96, "StagePhase layout");
struct StageKArgs {
    const StagePhase* phases;
    const void* weights;         // per phase [cu 32][wave 4][k-step][tile][lane 64][16 B]
    const void* prm;             // per phase, per 4 channels {scale[4], bias'[4], comp[4]}
    const void* zero;            // >= 16 zero bytes
    unsigned long long* sync;    // [8] registration counters, [8] arrival counters (one 128-byte line each), [16*16] abort flag
    int n_phases, n_barriers;
    int n_img, H, W;             // H * W <= 64
    unsigned long long* trace;   // diagnostics (saber_hip_stage_trace): [256 workgroups][n_phases][8] wall-clock stamps, or null
    void* t[STAGE_MAX_TENSORS];
};
bool stage_xcd_type(int tiles_per_cu, int ksteps_per_wave, int is3x3, int* type);
hipError_t launch_stage_xcd(const StageKArgs& a, size_t lds_bytes, hipStream_t s);
// the same phase code as an ordinary kernel: ONE conv (a.phases[0]), grid = n_img x 32 workgroups - workgroup (img, c) computes
// output channels [c * 16 NT, (c + 1) * 16 NT) of image img with the whole image in LDS and its weight slice in registers
hipError_t launch_img_conv(const StageKArgs& a, size_t lds_bytes, hipStream_t s);
// ONE 1x1 conv 512 -> (1537 .. 2048) channels on <= 64 pixels per image (+ eltwise) with the global average pooling of its output
// (conv1x1_gpool.hip): everything by value, no phase table. w / prm: the stage packing of that conv (nt = 4, 2 k-steps per wave)
struct GpoolKArgs {
    const void* x;               // [n_img][hw][512] 8-bit
    void* y;                     // [n_img][hw][cout] 8-bit
    const void* res;             // eltwise: [n_img][hw][cout] s8
    void* y_pool;                // [n_img][cout] 8-bit of y's dtype
    const void* w;
    const void* prm;
    const void* zero;            // >= 16 zero bytes
    int n_img, hw, cout;
    int in_u8, relu, out_u8, elt, res_relu;
    float coeff_conv, scale_conv, coeff_res, scale_res;
    float pool_idiv;
};
bool conv1x1_gpool_ok(int cin, int cout, int hw);
hipError_t launch_conv1x1_gpool(const GpoolKArgs& a, hipStream_t s);

// hipcc fetches kernel arguments lazily with scalar loads and places each load near its first use; every batch that is
// issued after an `s_waitcnt lgkmcnt(0)` is one more DEPENDENT round trip (~0.2-0.25 us, measured) before the kernel's
// first operand load. Naming the hot fields in one empty asm statement makes all of them live at that point, so their
// loads are issued together ahead of a single wait.
__device__ __forceinline__ void pin_hot_args(const ConvKArgs& a) {
    asm volatile("" ::"s"(a.x), "s"(a.w), "s"(a.zero), "s"(a.npx), "s"(a.nky), "s"(a.mg_npx), "s"(a.Kg_pad), "s"(a.M), "s"(a.OH),
                 "s"(a.OW), "s"(a.inv_ohw), "s"(a.inv_ow), "s"(a.H), "s"(a.W), "s"(a.C), "s"(a.stride_h), "s"(a.stride_w),
                 "s"(a.pad_h), "s"(a.pad_w), "s"(a.dil_h), "s"(a.dil_w), "s"(a.kh), "s"(a.kw), "s"(a.steps), "s"(a.in_u8));
}

// tile ids for launch_conv_igemm
enum { TILE_32x32 = 0, TILE_64x32 = 1, TILE_64x64 = 2, TILE_128x64 = 3, TILE_64x128 = 4, TILE_128x128 = 5,
       TILE_COUNT = 6,
       // FP32 bf16-plane kernels only (conv_igemm_impl.h NWM = 4): the same block tiles computed by 8 waves (two per SIMD)
       TILE_W8_64x64 = 6, TILE_W8_128x64 = 7, TILE_W8_128x128 = 8, TILE_W8_256x128 = 9, TILE_COUNT_B3 = 10 };
void tile_dims(int tile, int* bm_k, int* bn_pix);

// mode: 0 = int8 (C % 16 == 0), 1 = int8 C4 (input NHWC4), 2 = f32 (C % 4 == 0)
// ks: 64-byte MFMA k-steps per pipeline stage (1, 2 or 4)
hipError_t launch_conv_igemm(int mode, int tile, int ks, const ConvKArgs& a, hipStream_t s);
// LDS-DMA ring variant (modes 0 and 2 only)
hipError_t launch_conv_igemm_dma(int mode, int tile, int ks, int wg, const ConvKArgs& a, hipStream_t s);
// INT8 3x3 / stride 1 / dilation 1 / C % 64 == 0 with an LDS-resident input halo; th = 4 or 8 tile rows
hipError_t launch_conv3x3_halo(int th, const ConvKArgs& a, hipStream_t s);
// INT8 3x3 / stride 1 / C in {64,128,256,512} on small feature maps: image slabs (a.ib images x a.rb rows) resident in
// LDS, 16 output channels per workgroup with the weights in registers (conv3x3_img.h)
hipError_t launch_conv3x3_img(const ConvKArgs& a, int nw, int ib, int rb, hipStream_t s);
bool conv3x3_img_feasible(int C, int OW, int OH, int N, int nw, int ib, int rb);
// FP32 3x3 / stride 1 / pad 1 on the bf16 matrix cores with an LDS-resident input halo (conv3x3_b3h.hip); variant 1..5 = (output
// channels per workgroup, tile rows, 16-channel tiles per wave, threads): a.w = the fragment-ordered weight planes for that tm
bool conv3x3_b3h_variant(int variant, int* bmk, int* th, int* tm, int* threads);
// FP32 1x1 / stride 1 with C = 64 / 128 input channels: persistent independent waves, weight planes in registers (conv1x1_pw.hip)
bool conv1x1_pw_ok(int c, int k);
hipError_t launch_conv1x1_pw(const ConvKArgs& a, hipStream_t s);
// FP32 1x1 / stride 1 with C = 128 .. 2048 (C % 128 == 0): the four waves of a workgroup split the reduction, D slabs in flight per wave, no
// LDS staging (conv1x1_pwk.hip); variant 1 .. 4 -> (16-channel tiles, 16-pixel groups, slabs in flight, workgroups per CU)
bool conv1x1_pwk_variant(int v, int* tm, int* p, int* d, int* minb);
bool conv1x1_pwk_ok(int m, int c, int k);
hipError_t launch_conv1x1_pwk(int variant, const ConvKArgs& a, hipStream_t s);
hipError_t launch_conv3x3_b3h(int variant, const ConvKArgs& a, hipStream_t s);
// INT8 fc for <= 16 batch rows: 16 outputs per workgroup, reduction split over its 4 waves, operands loaded straight
// into MFMA registers (fc_small.hip). a.M rows, a.C reduction, a.K outputs, FC epilogues only.
hipError_t launch_fc_i8_small(const ConvKArgs& a, hipStream_t s);
bool fc_i8_small_ok(int m, int c, int kg_pad);
// the FP32 counterpart (EPI_F32 epilogue: + bias, optional relu), any a.C % 4 == 0
hipError_t launch_fc_f32_small(const ConvKArgs& a, bool packed, hipStream_t s);
int fc_f32_packed_steps(int c);
bool fc_f32_small_ok(int m, int c, int kg_pad);
bool fc_i8_small_softmax_ok(int m, int c, int kg_pad, int k);
hipError_t launch_fc_i8_small_softmax(const ConvKArgs& a, float* prob, unsigned* ctr, hipStream_t s);
// FP32 fc at <= 16 rows with the reduction split over workgroups (+ the Softmax over its output in the same launch when prob != null)
bool fc_f32_splitk_ok(int m, int c, int kg_pad, int k, bool softmax);
size_t fc_f32_splitk_part_floats(int c, int k);
size_t fc_f32_splitk_counters(int k);
hipError_t launch_fc_f32_splitk(const ConvKArgs& a, float* part, unsigned* ctr, float* prob, hipStream_t s);
bool gemm_f32_rows_ok(int m, int k);
hipError_t launch_gemm_f32_rows(int m, int n, int k, float alpha, const float* A, const float* B, float beta, float* C, const void* zero,
                                hipStream_t s);
// ResNet stem (7x7 stride 2, <= 4 channels) with the input patch in LDS; f32_in: fuse the quantise-on-entry
hipError_t launch_conv_stem(int f32_in, const ConvKArgs& a, hipStream_t s);
// ... followed by the 3x3 / stride-2 / pad-0 max pooling in the same kernel (s8 / u8 outputs only)
hipError_t launch_conv_stem_pool(int f32_in, const ConvKArgs& a, hipStream_t s);
hipError_t launch_conv_stem_pool_pair(int f32_in, const StemPairKArgs& a, hipStream_t s);
// Generic fallback: any C / group. w is OIHW-like repack [K][kh][kw][Cg]. mode 0 int8, 2 f32
hipError_t launch_conv_direct(int is_f32, const ConvKArgs& a, int group, hipStream_t s);
// Depthwise 3x3 (group == C == K, dilation 1, stride 1 | 2, pad 0 | 1, NHWC in / out, no residual; conv_dw3x3.hip): a lane owns a
// 16-byte channel vector (C % 16 == 0 for INT8, C % 4 == 0 for FP32). a.w = the weights as [tap][C]; form 1 = strips of 4 (FP32, "rows4") / 2 (INT8,
// "rows2") output rows per lane, form 2 = one output pixel per lane ("px"). Same bits as launch_conv_direct on these ops.
constexpr int DW3X3_FORMS = 2;
const char* conv_dw3x3_form_name(int form, bool f32);
bool conv_dw3x3_ok(bool f32, int n, int c, int k, int group, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                   int dil_w, int oh, int ow);
hipError_t launch_conv_dw3x3(int form, bool f32, const ConvKArgs& a, hipStream_t s);
// Grouped 3x3 INT8 on the i8 matrix cores (group > 1, Cg == Kg in {4, 8, 16, 32, 64}, C % 64 == 0, dilation 1, stride 1 | 2, pad 0 | 1, NHWC
// in / out, no residual; conv_group3x3.hip): a wave owns 16 output pixels x 64 output channels (form 1, "w16").
// a.w = the fragment-ordered planes of group3x3_pack, a.comp = 128 * sum(w[k]) for u8 input. Same bits as launch_conv_direct on these ops.
constexpr int G3X3_FORMS = 1;
const char* conv_group3x3_form_name(int form);
int conv_group3x3_steps(int cg);      // 64-byte K-steps per 16-channel row block
bool conv_group3x3_ok(int n, int c, int k, int group, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                      int oh, int ow);
hipError_t launch_conv_group3x3(int form, const ConvKArgs& a, int group, hipStream_t s);

// Depthwise 3x3 + pointwise 1x1 INT8 in one launch (MobileNet's separable pair; conv_sep.hip): a workgroup computes the depthwise conv of a
// tile of `rows` x 16 output pixels for all C channels into LDS and multiplies it on the i8 matrix cores with its slice of the pointwise
// conv's output channels. C % 32 == 0, 32 <= C <= 1024, K % 32 == 0.
struct SepKArgs {
    const void* x;        // the depthwise conv's input [N][H][W][C], s8 or u8
    const void* wdw;      // its weights [tap][C] s8
    const float* dw_bias; // its bias' [C] (never null: zeros stand for "no bias", (float)acc + 0.f == (float)acc)
    const float* dw_scale;
    const void* wpw;      // the pointwise conv's weights in fragment order (sep_pw_pack)
    const void* prm;      // the pointwise conv's {scale[4], bias'[4], comp[4]} per 4 output channels, padded to a multiple of 64 channels
    void* y_dw;           // [N][OH][OW][C] 8-bit, or null: the depthwise edge is not written
    void* y_pw;           // [N][OH][OW][K] 8-bit
    int N, H, W, C, OH, OW, K;
    int stride, pad;
    int tiles_x, tiles_per_img;   // 16-column tiles per tile row, tiles per image
    int kgroups;          // 64-channel groups of the pointwise conv per workgroup
    int nslices;          // workgroups per pixel tile (each recomputes the depthwise tile): ceil(K / 64 / kgroups)
    int dw_relu, mid_u8;  // the depthwise conv's relu and output type (= the pointwise conv's input type)
    int pw_relu, out_u8;
};
// the table of launch forms: code 1 .. 15 -> pixel rows per tile, output channels per workgroup (0: all of them), waves per workgroup; false: no
// such form. sep_form_ok: the form exists and fits this pair (a form that splits K needs more than one slice)
constexpr int SEP_MAX_CODE = 15;
bool conv_sep_form(int code, int* rows, int* kper, int* waves);
bool conv_sep_form_ok(int code, int c, int k);
size_t conv_sep_lds_bytes(int rows, int c);
void sep_pw_pack(const int8_t* w_kc, int k, int c, std::vector<uint8_t>& out);      // [ceil(K / 64)][ceil(C / 64)][4][64 lanes][16], zero padded
hipError_t conv_sep_prepare();      // per device, once: the kernels may use more than 64 KB of LDS
hipError_t launch_conv_sep(int code, bool in_u8, const SepKArgs& a, hipStream_t s);

// Inverted-residual block (MobileNet-v2): 1x1 expand + depthwise 3x3 + 1x1 linear project (+ the eltwise sum with the block's input) INT8 in
// one launch (conv_ir.hip). A workgroup owns a tile of output pixels of one image and ALL of Cout; per chunk of 64 expanded channels it
// expands the tile's input halo on the i8 matrix cores into LDS, runs the depthwise conv from there into LDS and adds one k-step of the
// project conv to accumulators that live across the chunks. Cin % 8 == 0, 8 <= Cin <= 192, Ce % 16 == 0, Ce <= 1024, Cout % 8 == 0, Cout <= 320.
struct IrKArgs {
    const void* x;        // [N][H][W][Cin] s8 | u8
    const void* we;       // the expand conv's weights in fragment order (ir_pack of [Ce][Cin])
    const void* eprm;     // its {scale[4], bias'[4], comp[4]} per 4 channels, padded to a multiple of 64 channels
    const void* wdw;      // the depthwise conv's weights [tap][Ce] s8
    const float* dw_bias; // its bias' [Ce] (zeros stand for "no bias") and scale [Ce]
    const float* dw_scale;
    const void* wp;       // the project conv's weights in fragment order (ir_pack of [Cout][Ce])
    const void* pprm;     // its {scale[4], bias'[4], comp[4]} per 4 channels, padded to a multiple of 64 channels
    void* y_e;            // [N][H][W][Ce] u8, or null: the expanded edge is not written
    void* y_d;            // [N][OH][OW][Ce] u8, or null: the depthwise edge is not written
    void* y;              // [N][OH][OW][Cout] s8 | u8
    int N, H, W, Cin, Ce, OH, OW, Cout;
    int stride;           // of the depthwise conv (1 | 2; pad 1)
    int th, tw, nf;       // the tile: th x tw output pixels in nf = ceil(th * tw / 16) fragments of 16 (pixel p = row p / tw, column p % tw)
    int hh, hw, hpf;      // its input halo: ((th - 1) * stride + 3) x ((tw - 1) * stride + 3) pixels in hpf fragments of 16
    int tiles_x, tiles_per_img;
    int out_u8, p_relu;   // the project conv's output type and relu (without the eltwise)
    int elt, res_relu;    // the fused eltwise with x as the residual (s8, Cin == Cout, stride 1); relu after the sum
    float coeff_conv, scale_conv, coeff_res, scale_res;
};
// the launch forms: code 1 .. IR_MAX_CODE -> the tile of a block of this shape, false: no such form for it (or its LDS footprint is above
// IR_LDS_LIMIT: two workgroups per CU must fit)
constexpr int IR_MAX_CODE = 7;
constexpr int IR_MAX_UNITS = 20;      // (64 output channels x 16 pixels) accumulator units per workgroup: 5 per wave
constexpr size_t IR_LDS_LIMIT = 80 * 1024 - 64;
struct IrGeom { int th, tw, nf, hh, hw, hpf, tiles_x, tiles_y; size_t lds; };
const char* conv_ir_form_name(int code);      // "" where the table has no such code
bool conv_ir_geom(int code, int cin, int ce, int cout, int oh, int ow, int stride, IrGeom* g);
void ir_pack(const int8_t* w_kc, int k, int c, std::vector<uint8_t>& out);      // [ceil(K / 64)][ceil(C / 64)][4][64 lanes][16], zero beyond K and beyond C
hipError_t conv_ir_prepare();      // per device, once: the kernels may use more than 64 KB of LDS
hipError_t launch_conv_ir(int code, bool in_u8, const IrKArgs& a, hipStream_t s);      // sets the tile fields of `a` from the form

// SqueezeNet's Fire module - a 1x1 squeeze conv (C -> S), the 1x1 (S -> E1) and the padded 3x3 (S -> E3) expand convs that both read it, and the
// channel concat of the two - INT8, in one launch (conv_fire.hip). A workgroup owns a tile of pixels of one image and ALL of E1 + E3: it squeezes
// the tile and a one-pixel halo on the i8 matrix cores into LDS (S padded to one 64-deep k-step), runs both expand convs from there and stores
// each into its channel slice of the one output tensor. ACCEPTED: S in {16, 32, 48, 64}; C, E1, E3 multiples of 16, 16 <= C <= 512,
// 16 <= E1, E3 <= 512; x s8 | u8; the three convs relu -> u8; stride 1, dilation 1, group 1, the 3x3 with pad 1.
struct FireKArgs {
    const void* x;        // [N][H][W][C] s8 | u8
    const void* ws;       // the squeeze conv's weights in fragment order (ir_pack of [S][C])
    const void* sprm;     // its {scale[4], bias'[4], comp[4]} per 4 channels, padded to 64 channels
    const void* w1;       // the 1x1 expand conv's weights (ir_pack of [E1][S]: one k-step)
    const void* prm1;
    const void* w3;       // the 3x3 expand conv's weights: per tap (ir_pack of [E3][S]) - nine k-steps, [tap][group of 64][4][64 lanes][16]
    const void* prm3;
    void* y_s;            // [N][H][W][S] u8, or null: the squeeze edge is not written
    void* y;              // [N][H][W][E1 + E3] u8: expand1x1 at channel 0, expand3x3 at channel E1
    int N, H, W, C, S, E1, E3;
    int th, tw, nf;       // the tile: th x tw pixels in nf fragments of 16
    int hh, hw, hpf;      // its halo: (th + 2) x (tw + 2) pixels in hpf fragments of 16
    int tiles_x, tiles_per_img;
};
// the launch forms: code 1 .. FIRE_MAX_CODE -> the tile; false: no such form for this shape, the shape is outside the accepted range, or the
// LDS footprint is above FIRE_LDS_LIMIT
constexpr int FIRE_MAX_CODE = 2;
constexpr size_t FIRE_LDS_LIMIT = 80 * 1024 - 64;
struct FireGeom { int th, tw, nf, hh, hw, hpf, tiles_x, tiles_y; size_t lds; };
const char* conv_fire_form_name(int code);      // "" where the table has no such code
bool conv_fire_geom(int code, int c, int s, int e1, int e3, int h, int w, FireGeom* g);
hipError_t conv_fire_prepare();
hipError_t launch_conv_fire(int code, bool in_u8, const FireKArgs& a, hipStream_t s);      // sets the tile fields of `a` from the form

// FP32 transposed convolution (deconv.hip). x [N, C, H, W] logical, w: direct kernel = the weights repacked to [tap][C][K / group],
// wfrag: the bf16-plane kernels' fragment stream (deconv_b3_pack), y [N, K, OH, OW] logical; gather kernels, no workspace.
struct DeconvKArgs {
    const float* x;
    const float* w;
    const void* wfrag;
    const float* bias;    // [K] or null
    float* y;
    int N, H, W, C, K, OH, OW;
    int kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, group;
    int in_nchw, out_nchw, relu;
    int q0_h, q0_w, tiles_y, tiles_x;      // deconv_b3: first cell row / column, cell tiles per image (set by the launcher)
};
hipError_t launch_deconv_direct_f32(const DeconvKArgs& a, hipStream_t s);
// the bf16-plane kernel: group 1, dilation 1, stride 2 x 2, kh == kw in {2, 3, 4}, pad <= k - 1, C % 32 == 0, K % 16 == 0, NHWC in and out;
// form 1 = 4 x 16 cells per workgroup, 2 = 2 x 16 (a cell = the 2 x 2 output pixels of the four phases); same bits in both
constexpr int DECONV_B3_FORMS = 2;
bool deconv_b3_form(int form, int* th);
bool deconv_b3_ok(int n, int h, int w, int c, int k, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int group);
int deconv_b3_taps(int ks, int (*ab)[2]);      // the stream's [phase][tap] order as (a, b) pairs; returns ks * ks
void deconv_b3_pack(const float* w_ckab, int c, int k, int ks, std::vector<uint8_t>& out);      // [phase][tap][slab][tile][plane][lane] x 16 B
hipError_t launch_deconv_b3_f32(int form, const DeconvKArgs& a, hipStream_t s);

// FP32 resize (resize.hip). x [N, C, H, W] logical, y [N, C, OH, OW] logical; th / tw: DEVICE tables of OH / OW entries (which input rows /
// columns an output row / column reads and with which fraction), made on the host by resize_axis_table in the reference's float steps.
struct ResizeTap {
    int i0, i1;      // the two taps' indices; i1 >= the input size reads as 0 (RESIZE_CUSTOM); nearest: i0 == i1 = the one tap
    float frac;      // f - float(i0)
    int pad;
};
struct ResizeKArgs {
    const float* x;
    const float* b;      // the fused sum's second operand (the output's shape and layout) or null: y = relu?(c0 * resize(x) + c1 * b)
    float* y;
    const ResizeTap* th;
    const ResizeTap* tw;
    int N, C, H, W, OH, OW;
    int nearest, in_nchw, out_nchw, relu;
    float c0, c1;
};
// mode 0 BILINEAR_ALIGN, 1 BILINEAR_NO_ALIGN, 2 RESIZE_CUSTOM (scale = the param's scale unless sizes_given), 3 NEAREST_ALIGN; false: a
// descriptor the reference cannot run (modes 0 / 3 to one output row, a tap at or beyond the input, no positive scale)
bool resize_axis_table(int mode, int in, int out, float scale, bool sizes_given, std::vector<ResizeTap>& t);
bool resize_rows_ok(int c, int in_nchw, int out_nchw);      // form 1: NHWC on both sides, c % 4 == 0
bool resize_x2_tables_ok(bool nearest, int in, const std::vector<ResizeTap>& t);      // form 2: one axis of an integer x2 whose taps stay within a row of o / 2
// form 0 resize_direct_f32 (every descriptor), 1 resize_rows_f32, 2 resize_x2_f32; the same bits in all, with and without the fused sum
hipError_t launch_resize_f32(int form, const ResizeKArgs& a, hipStream_t s);

// FP32 DetectionOutput (detout.hip): box decode, per-class NMS and the per-image keep_top_k cut in two launches, fixed-shape output.
constexpr int DETOUT_SORT_CAP = 4096;            // 64-bit keys one workgroup sorts in LDS at a time (both forms, and the per-image cut)
constexpr int DETOUT_MAX_NMS_TOP_K = 1024;       // the survivors of one (image, class): boxes, and form 1's K x K / 64 bit matrix, stay in LDS
constexpr size_t DETOUT_LDS_LIMIT = 160 * 1024 - 64;
struct DetoutKArgs {
    const float* loc;        // [N, P * 4]: the predictions (prior != null) or decoded boxes
    const float* conf;       // prior != null: [N, P, C] (what the softmax writes); else [N, C, P]
    const float* prior;      // [2, P * 4]: boxes, then variances; or null
    float* y;                // [N * keep, 7]
    int* count;              // [1 + N]
    int* cls_cnt;            // scratch [N * C]: how many candidates NMS kept per (image, class)
    uint2* cls_key;          // scratch [N * C * K]: their score bits and prior index, in the order they were kept
    float4* cls_box;         // scratch [N * C * K]: their boxes
    int N, C, P, K, keep, bg;      // K = nms_top_k
    int code, vit;           // CodeType 1 CORNER, 2 CENTER_SIZE, 3 CORNER_SIZE; variance_encode_in_target
    float conf_t, nms_t, eta;
    int region0;             // (set by the launcher)
};
// the per-image cut selects in LDS: keep_top_k fits beside one step of new keys, or is so large that no image can exceed it
inline bool detout_keep_fits(int C, int K, long long keep) { return keep <= DETOUT_SORT_CAP - 1024 || keep >= (long long)C * K; }
size_t detout_lds_bytes(int form, int K);      // dynamic LDS of launch 1
// form 0 detout_direct_f32 (any eta), 1 detout_mask_f32 (eta == 1); then detout_pack_f32. The same bits from both forms.
hipError_t launch_detout_f32(int form, const DetoutKArgs& a, hipStream_t s);

// reads `bytes` of device memory through every XCD (autotuning: the timed launch then finds none of its operands in
// an L2, which is how it runs inside the op list)
hipError_t launch_l2_flush(const void* buf, size_t bytes, unsigned* sink, hipStream_t s);

// elementwise / layout / pooling / softmax (elementwise.hip)
hipError_t launch_quantize_nchw_to_nhwc(int n, int c, int h, int w, int c_pad, int out_dtype, float scale,
                                        const float* x, void* y, hipStream_t s);
hipError_t launch_dequantize_nhwc_to_nchw(int n, int c, int h, int w, int in_dtype, float scale, const void* x,
                                          float* y, hipStream_t s);
hipError_t launch_transpose_nchw_to_nhwc_f32(int n, int c, int h, int w, int c_pad, const float* x, float* y,
                                             hipStream_t s);
hipError_t launch_transpose_nhwc_to_nchw_f32(int n, int c, int h, int w, int c_pad, const float* x, float* y,
                                             hipStream_t s);
hipError_t launch_pad_channels_i8(size_t pixels, int c, int c_pad, const void* x, void* y, hipStream_t s);
// bytes [rows][cols] -> [cols][rows_pad] (zero filled beyond rows): op(A) = A^T staging of the INT8 GEMM
hipError_t launch_transpose_bytes(int rows, int cols, int rows_pad, const void* x, void* y, hipStream_t s);
hipError_t launch_quantize_flat_s8(size_t count, float scale, const float* x, int8_t* y, hipStream_t s);
hipError_t launch_eltwise_sum_i8(size_t count, const int8_t* a, const int8_t* b, float sa, float sb, float c0,
                                 float c1, int relu, int8_t* y, hipStream_t s);
hipError_t launch_eltwise_sum_f32(size_t count, const float* a, const float* b, float c0, float c1, int relu,
                                  float* y, hipStream_t s);
hipError_t launch_relu_f32(size_t count, const float* x, float* y, hipStream_t s);
// concat along the channel axis of up to CONCAT_MAX_INPUTS NHWC tensors: rows of row_bytes[i] bytes per pixel, copied (mult NULL or 1) or - u8 -
// rescaled by mult[i]
constexpr int CONCAT_MAX_INPUTS = 8;
struct ConcatKArgs {
    const void* x[CONCAT_MAX_INPUTS];
    int cb[CONCAT_MAX_INPUTS], off[CONCAT_MAX_INPUTS], unit[CONCAT_MAX_INPUTS];      // row bytes, byte offset in the output row, bytes per lane (16 | 4 | 1)
    float m[CONCAT_MAX_INPUTS];
    int ctot;                                                                         // output row bytes
};
hipError_t launch_concat_nhwc(size_t pixels, int n_inputs, const void* const* xs, const int* row_bytes, const float* mult, void* y, hipStream_t s);
hipError_t launch_activation_f32(int active, size_t count, float slope, float coef, const float* x, float* y, hipStream_t s);
hipError_t launch_prelu_f32(size_t count, int channels, int inner, int shared, const float* slope, const float* x, float* y, hipStream_t s);
hipError_t launch_pool2d_i8_nhwc(int n, int h, int w, int c, int oh, int ow, int kh, int kw, int sh, int sw,
                                 int ph, int pw, int type, int in_dtype, int out_dtype, const void* x, void* y,
                                 hipStream_t s);
hipError_t launch_pool2d_f32(int n, int h, int w, int c, int oh, int ow, int kh, int kw, int sh, int sw, int ph,
                             int pw, int type, int nchw, const float* x, float* y, hipStream_t s);
hipError_t launch_pool2d_f32_from_i8(int n, int h, int w, int c, int oh, int ow, int kh, int kw, int sh, int sw, int ph,
                                     int pw, int type, int in_dtype, float scale, const void* x, float* y,
                                     float q_scale, int8_t* yq, hipStream_t s);   // yq: optional fused s8 quantisation
hipError_t launch_softmax_f32(int rows, int cols, const float* x, float* y, hipStream_t s);
hipError_t launch_xcd_map_probe(unsigned* out, int blocks, hipStream_t s);   // out[b] = XCD of workgroup b
hipError_t launch_gemm_f32(int ta, int tb, int m, int n, int k, float alpha, const float* a, const float* b,
                           float beta, float* c, hipStream_t s);

// FP32 stem: NCHW f32 image -> conv 7x7 / 2 / pad 3 (3 -> 64) + bias + relu -> max pooling 3x3 / 2 -> NHWC f32, one launch (conv_stem_f32.hip)
struct StemF32Args;
void stem_f32_pack(const float* w_oihw, std::vector<uint8_t>& out);
void group3x3_pack(const int8_t* q_oihw, int c, int cg, std::vector<uint8_t>& out);      // conv_group3x3.hip: [C / 64][4][steps][64 lanes][16]
hipError_t launch_conv_stem_f32_pool_raw(const float* x, const void* w, const float* bias, float* y, int n, int h, int w_, int oh, int ow, int ph,
                                         int pw, int variant, hipStream_t s);
}  // namespace saber_mi355x
