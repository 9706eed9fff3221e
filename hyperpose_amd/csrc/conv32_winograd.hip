// conv32_winograd.hip — the 3 x 3, stride-1 convolutions of the fp32 engine (HP_DTYPE_F32, data_type::kFLOAT) in Winograd's minimal form
// F(2 x 2, 3 x 3) on the fp32 matrix pipe (interface: conv_fp32.hpp).
//
// The fp32 pipe (v_mfma_f32_16x16x4_f32: 64 FLOP/clk/SIMD, 157 TFLOP/s) is the bound of every dense fp32 layer here, so the lever left is the
// number of multiplications.  For a 2 x 2 output tile and a 3 x 3 filter (Lavin & Gray; what cuDNN / TensorRT pick for fp32 3 x 3 layers - the
// reference's engine, src/tensorrt.cpp:327-353, leaves the choice to the TensorRT builder):
//        Y = At [ (G g Gt) . (Bt d B) ] A            d: the 4 x 4 input patch, g: the filter, ".": element-wise, summed over input channels
//        Bt = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]    At = [1 1 1 0; 0 1 -1 -1]
// i.e. 16 multiplications per tile and channel pair instead of 36: the sum over input channels is 16 independent matrix products
//        M[pos][cout][tile] = sum_c U[pos][cout][c] V[pos][c][tile]          U = G g Gt (host, once),  V = Bt d B (per launch, in LDS)
// - 2.25 x fewer MFMA cycles than the direct form.  Input and output transforms are additions only; U's factors 1/2 and 1/4 are exact in binary
// and U is rounded to fp32 once on the host (computed in double).  The products and sums of the 16 matrix products are exact fp32 FMAs on the
// matrix pipe like everywhere else in this engine; what changes against the direct form is the order of summation and the cancellation inside the
// transforms - measured against the pure fp32 oracle in tests/test_engine_fp32_gpu.py (same 1e-4 bound as every fp32 kernel; DESIGN.md 7 has the
// measured figures).
//
// Kernel shape (MW = wavefronts per block, 4 by default):
//   block   = 16 x 8 output pixels = 8 x 4 Winograd tiles (two N = 16 column tiles of the MFMA) x 16 MW output channels; a wavefront = ONE
//             16-row MFMA tile of channels x 32 tiles x 16 positions = 128 accumulator registers.  MW = 4: two blocks per CU - one block's
//             transform phases and epilogue run under the other's MFMAs; MW = 8 (measured, no longer launched): one block of two wavefronts per SIMD per
//             CU, the staging / transform of a pixel tile shared by 128 channels - 44.6 us alone against 46.3 for a 128 -> 128 layer at
//             8 x 46 x 54, but 31.5 against 28.8 with a second stream (its phases are in step inside the one block).
//             (The first form - 32 channels x 16 tiles per wavefront - read 2 KB of A per eight MFMAs: 68 us alone.)
//   K loop  = chunks of 16 input channels.  The chunk's 18 x 10 halo patch (19 rows in a block that holds an image boundary: see "rows form" in
//             the kernel) arrives from HBM as fp32 (requested two chunks ahead, into registers), goes to LDS, is
//             transformed cooperatively (a wavefront = ONE row of Bt d B for 16 tiles, lane = (tile, 4-channel
//             quad): 8 LDS reads, 8 vector additions, 4 LDS writes) into V[pos][tile][16 channels].  MW = 4 (PIPE): two V buffers, the
//             transform of chunk c + 1 cut into 16 pieces that sit inside the 16 MFMA steps of chunk c (46.6 -> 44.3 us alone, 28.9 -> 27.0
//             with a second stream; the unpipelined form is no longer launched); MW = 8: one buffer, the transform between two barriers;
//   MFMA    = per position one step of 16 channels: lane (row / tile, kq) holds channels 4 kq .. 4 kq + 3 of its row (A, 1 KB from L2 in
//             fragment order, six steps ahead) / tile (B, two ds_read_b128 from V) and feeds element e to MFMA e - 8 MFMAs of 32 cycles per step;
//   output  = bias, slopes and the residual quads of all of the wavefront's pixel rows are requested right behind the K loop; then At M A per
//             lane from its own registers (lane (tile, kq) holds channels 4 kq + r at all 16 positions), written into a slab the block shares
//             ([128 pixels][16 MW channels]), then the row-major epilogue (the arithmetic of conv32_epilogue.hpp): whole pixel rows, the stores
//             of all passes back to back.
// Block timeline (tools/direct_timeline.py f32; shader cycles at 2.2 GHz, MW = 4, PIPE, 128 -> 128 at 8 x 46 x 54, 322 blocks, two per CU; medians
// of 34 launches, profiles/winograd_phases.json): chunk 0 staged 2.5 k | transformed, chunk 1's patch stored 2.6 k | per chunk: multiplied 7.2 -
// 8.7 k (chunk 0: 6.4 k; 8.2 k = the pipe's time for the two blocks' 2 x 128 MFMAs per SIMD: the loop is at the pipe's rate), next patch stored
// 0.4 - 1.0 k | epilogue requests 2.1 k (3.1 k with a residual) | output transform 1.5 k | stores 5.4 k.  81 - 82 k cycles per block, with or
// without a residual (before: 85 k without, 89 k with one), of which 2 x 32.8 k are MFMA issue.
#include "conv32_pick.hpp"

#include "conv32_epilogue.hpp"
#include "conv_device.hpp"

#include <cstdlib>
#include <vector>

namespace hp {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat; // global memory, said to the compiler
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// (WCK = 16, the input channels per chunk: conv32_pick.hpp)
constexpr int HALO_W = 10;                     // halo patch of the 16 NC x 8 pixel tile: (8 NC + 2) x 10 pixels
constexpr int RAW_PB = WCK * 4;
constexpr int VP = 24 * 4;                     // V row (one tile, 16 channels) pitch in bytes: 24 floats - the transform's ds_write_b128 and the MFMA's ds_read_b128 are conflict-free

// NC = 16-tile MFMA column tiles per block and wavefront: 2 = a block of 16 x 8 pixels (8 x 4 tiles), 1 = 8 x 8 pixels (4 x 4 tiles)
template <int MW, int NC = 2>
struct wino_geom {
    static constexpr int NT = 64 * MW;
    static constexpr int TB = 4 * NC;                 // tile rows of a block
    static constexpr int HALO_H = 8 * NC + 2;         // patch rows of a block inside one image
    static constexpr int PATCH_H = HALO_H + 1;        // ... of a block that holds an image boundary (rows form, even H): the tiles at the boundary share one row
    static constexpr int RAW_Q = PATCH_H * HALO_W * 4; // float4 quads of the halo patch (64 bytes per pixel): 760 | 440
    static constexpr int NQ = (RAW_Q + NT - 1) / NT;  // quads per thread and chunk
    static constexpr int RAW_BYTES = NQ * NT * 16;    // + room for the surplus threads' (discarded) quads: the store to LDS has no branch
    static constexpr int NI = 4 * NC / MW;            // transform items (row of Bt d B, 16 tiles) per wavefront and chunk
    static_assert(NI >= 1, "a transform item per wavefront");
    static constexpr int TMS = MW / 2;                // the block's output slab: [64 NC pixel rows][16 MW channels + 4] = rows_geom<TMS>
    static constexpr int SLAB_PITCH = rows_geom<TMS>::PITCH, SLAB_BYTES = 64 * NC * SLAB_PITCH * 4;
    static constexpr int VPOS = 16 * NC * VP, VBUF = 16 * VPOS; // one position (16 NC tiles), all 16 positions
    static constexpr int LDS_BYTES = RAW_BYTES + (VBUF > SLAB_BYTES ? VBUF : SLAB_BYTES);
    // the pipelined form (MW = 4): two V buffers without padding - 64 bytes per tile, the 16-byte quad index XOR-ed with a function of the
    // tile so that the transform's ds_write_b128 and the MFMA's ds_read_b128 (same lane -> (tile, quad) map) stay conflict-free
    static constexpr int PVPOS = 16 * NC * 64, PVBUF = 16 * PVPOS;                  // 32768 | 16384 bytes per buffer
    static constexpr int PLDS_BYTES = RAW_BYTES + (2 * PVBUF > SLAB_BYTES ? 2 * PVBUF : SLAB_BYTES); // 12288 + 65536 = 77824: two blocks per CU
};

__device__ __forceinline__ long tvw_off(const tview32& t, int b, int y, int x)
{
    return ((long)b * t.img + (long)y * t.wp + x) * t.cs + t.coff;
}

} // namespace

// PIPE: the input transform of chunk c + 1 runs inside the MFMA steps of chunk c (two V buffers): see "K loop" above
template <int MW, bool PIPE, int NC = 2>
__global__ __launch_bounds__(64 * MW, MW == 8 ? 1 : NC == 1 ? 3 : 2) void conv32_winograd_kernel(const conv32_params p, int tiles_x, int tiles_y, int vh, int T)
{
    static_assert(!PIPE || MW == 4, "the pipelined form is the four-wavefront one");
    using G = wino_geom<MW, NC>;
    constexpr int NT = G::NT, NQ = G::NQ, SLAB_PITCH = G::SLAB_PITCH, VPOS = G::VPOS;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[]; // G::LDS_BYTES
    unsigned char* const raw = lds;
    unsigned char* const vb = lds + G::RAW_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware block order (1-D grid): block id -> XCD id % 8; the NG channel groups of one pixel tile are ids b, b + 8, .. - back to back on one
    // XCD, whose L2 then serves the tile's halo patch NG - 1 times (conv_fp32.hip has the measurement behind this)
    // vh > 0, the "tall" form: the batch as ONE image of (B - 1) vh + H rows - an image's rows plus its halo rows are vh (even) rows of the buffer,
    // the halo rows between two images are zeros, i.e. the padding both of them need.  Tiles then run down the whole batch: a 12 x 12 map is
    // 14 rows of a 446-row image (28 blocks of 16 rows) instead of one three-quarters-empty block per image (32).  vh is even, so every 2 x 2
    // Winograd tile covers the same rows of every image: the same bits as the per-image form, whatever the batch.  Output rows that fall on
    // separator rows are computed and not stored.
    // T > 0, the "rows" form: tile rows numbered per image - T = ceil(H / 2) of them each, tile row r = rows 2 (r % T), 2 (r % T) + 1 of image
    // r / T - so the grid holds the B T tile rows that exist and no separator rows (8 x 23 = 184 tile rows are 23 blocks of 16 pixel rows, not
    // 24).  T >= the block's tile rows: a block holds at most one image boundary, after its first kb tile rows.  The tile row below the boundary
    // needs a row of zeros (its image's top halo row) and then its rows 0 - 2, the tile row above it ends with rows H - 2, H - 1, the bottom halo
    // row H (zeros) and, where H is odd, a fourth row that only feeds an output row that does not exist.  One halo row is as good as the other:
    // even H - the lower tile row starts ON the upper one's last patch row (the bottom halo row) and goes on with its own rows 0 - 2: a patch of
    // G::PATCH_H = G::HALO_H + 1 rows, the lower tile rows one patch row further down; odd H - it starts on the upper one's third row (the bottom
    // halo row) and its row 0 takes the place of the row nobody needs: G::HALO_H rows, no shift at all.  The same tiles of every image, the same
    // arithmetic on the same values: the same bits as the per-image form.
    const int NG = p.Cout_pad / (16 * MW), ntiles = tiles_x * tiles_y * (vh || T ? 1 : p.B);
    const int Hin = vh ? (p.B - 1) * vh + p.H : p.H; // rows 0 .. Hin - 1; row Hin = the (last) image's bottom halo row
    const int bj = blockIdx.x >> 3, by = bj % NG;
    int t = (bj / NG) * 8 + (blockIdx.x & 7);
    if (t >= ntiles)
        return; // (the grid is padded to whole groups of eight pixel tiles)
    const int bx = t;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int y0 = ty * (8 * NC), x0 = tx * 8;
    const int MT = p.Cout_pad / 16, mt = by * MW + wave;
    const int nch = p.Cin / WCK;
    int dbg_i = 0;
#define HP_STAMP()                                                     \
    if (p.dbg && bx == 1 && by == 0 && tid == 0)       \
        p.dbg[dbg_i++] = __builtin_amdgcn_s_memtime();
    HP_STAMP();
    if (p.dbg && bx == 1 && by == 0 && tid == 0)
        p.dbg[119] = __builtin_readcyclecounter(), p.dbg[120] = __builtin_amdgcn_s_memrealtime();

    // ---- staging geometry: quad q of a chunk = (halo pixel q / 4, channels 4 (q % 4) ..); halo pixel (hy, hx) = image pixel (y0 - 1 + hy, x0 - 1 + hx).
    // The tensor's zero halo is the convolution's padding; pixels further out (ragged last tiles, the fourth patch row / column of an odd-sized
    // map) are clamped to it and zeroed - they only feed outputs that are never stored
    // Rows form: patch rows 0 .. ylow - 1 are rows ly0 .. of image img0 (down to its bottom halo row), patch rows from ylow on are rows 0 .. of
    // image img0 + 1, whose tile rows start at patch row 2 j + sh (kb = TB: no boundary in this block); tile rows past the last image read
    // zeros.  The other forms: one run of rows (kb = TB) of image b
    int kb = G::TB, sh = 0, img0 = b, ly0 = y0 - 1, l0 = 0;
    if (T) {
        const int r0 = ty * G::TB;
        img0 = r0 / T, l0 = r0 - img0 * T, ly0 = 2 * l0 - 1;
        kb = min(T - l0, G::TB), sh = kb < G::TB && !(p.H & 1);
    }
    const int Hlim = T ? p.H : Hin, ylow = kb < G::TB ? 2 * kb + 1 + sh : G::PATCH_H;
    const int nvalid = (G::HALO_H + sh) * HALO_W * 4; // the quads this block needs
    long goff[NQ];
    bool qok[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = min(tid + i * NT, nvalid - 1);
        const int hp = q >> 2, c4 = q & 3;
        const int hy = hp / HALO_W, hx = hp - hy * HALO_W;
        const bool below = hy >= ylow;
        const int bi = below ? img0 + 1 : img0, y = below ? hy - ylow : ly0 + hy, x = x0 - 1 + hx;
        qok[i] = y <= Hlim && x <= p.W && bi < p.B;
        goff[i] = tvw_off(p.in, min(bi, p.B - 1), min(y, Hlim), min(x, p.W)) + c4 * 4;
    }
    f32x4 stage[NQ];
    auto gload = [&](int c) {
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            stage[i] = *reinterpret_cast<const f32x4*>(p.in.p + goff[i] + min(c, nch - 1) * WCK);
    };
    auto to_lds = [&]() { // (no branch: with one, hipcc drains EVERY load in flight - the A fragments of the next steps too - before the first store)
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            *reinterpret_cast<f32x4*>(raw + (tid + i * NT) * 16) = qok[i] ? stage[i] : f32x4{ 0.f, 0.f, 0.f, 0.f };
    };
    // the patch row of a block's tile row: two rows per tile row, and sh more below the image boundary (rows form)
    auto tile_src = [&](int tile, int quad) {
        const int tr = tile >> 2;
        return raw + ((2 * tr + (tr >= kb ? sh : 0)) * HALO_W + 2 * (tile & 3)) * RAW_PB + quad * 16;
    };
    // ---- input transform: item of a wavefront = (row i of Bt d B, 16 of the 32 tiles); lane (tile, quad) like the MFMA's B read.  Row i of
    // T = Bt d combines two patch rows; V[i][.] = T[i][.] B
    auto transform = [&]() {
#pragma unroll
        for (int k = 0; k < G::NI; ++k) {
            const int item = wave + k * MW, i = NC == 2 ? item >> 1 : item;
            const int quad = lane >> 4, tile = (NC == 2 ? (item & 1) * 16 : 0) + (lane & 15);
            const int ra = i == 0 ? 0 : i == 2 ? 2 : 1, rb = i == 0 ? 2 : i == 1 ? 2 : i == 2 ? 1 : 3;
            const float sg = i == 1 ? 1.f : -1.f;
            const unsigned char* const src = tile_src(tile, quad);
            f32x4 Td[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(src + (ra * HALO_W + j) * RAW_PB);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(src + (rb * HALO_W + j) * RAW_PB);
                Td[j] = a + sg * bq; // (an exact sign change, then one rounded addition)
            }
            constexpr int PS = PIPE ? G::PVPOS : VPOS;
            unsigned char* const dst = PIPE ? vb + (i * 4) * PS + tile * 64 + ((quad ^ ((4 - (tile >> 2)) & 3)) * 16) : vb + (i * 4) * PS + tile * VP + quad * 16;
            *reinterpret_cast<f32x4*>(dst) = Td[0] - Td[2];
            *reinterpret_cast<f32x4*>(dst + PS) = Td[1] + Td[2];
            *reinterpret_cast<f32x4*>(dst + 2 * PS) = Td[2] - Td[1];
            *reinterpret_cast<f32x4*>(dst + 3 * PS) = Td[1] - Td[3];
        }
    };
    // the same transform in pieces, one per MFMA step (PIPE): item k = 0 in steps 0 - 7, k = 1 in steps 8 - 15 of the PREVIOUS chunk's
    // multiplication: steps 0 - 3 read a column pair each, step 4 forms T, steps 4 - 7 form and store one position each
    f32x4 ta[4], tb[4];
    auto transform_piece = [&](int pos, int buf) {
        const int k = pos >> 3, ps = pos & 7;
        if (k >= G::NI)
            return; // (NC = 1: one item per wavefront, in steps 0 - 7)
        const int item = wave + k * MW, i = NC == 2 ? item >> 1 : item;
        const int quad = lane >> 4, tile = (NC == 2 ? (item & 1) * 16 : 0) + (lane & 15);
        const int ra = i == 0 ? 0 : i == 2 ? 2 : 1, rb = i == 0 ? 2 : i == 1 ? 2 : i == 2 ? 1 : 3;
        const unsigned char* const src = tile_src(tile, quad);
        if (ps < 4) {
            ta[ps] = *reinterpret_cast<const f32x4*>(src + (ra * HALO_W + ps) * RAW_PB);
            tb[ps] = *reinterpret_cast<const f32x4*>(src + (rb * HALO_W + ps) * RAW_PB);
        } else {
            if (ps == 4) {
                const float sg = i == 1 ? 1.f : -1.f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    ta[j] = ta[j] + sg * tb[j];
            }
            unsigned char* const dst = vb + buf * G::PVBUF + (i * 4 + (ps - 4)) * G::PVPOS + tile * 64 + ((quad ^ ((4 - (tile >> 2)) & 3)) * 16);
            *reinterpret_cast<f32x4*>(dst) = ps == 4 ? ta[0] - ta[2] : ps == 5 ? ta[1] + ta[2] : ps == 6 ? ta[2] - ta[1] : ta[1] - ta[3];
        }
    };

    // ---- A fragments: [chunk][pos][16-row tile][lane][4 floats]; step s = chunk * 16 + pos
    const long step_stride = (long)MT * 256;
    const float* const wp = p.w_wino + (long)mt * 256 + lane * 4;
    const int nsteps = nch * 16;
    constexpr int RING = PIPE ? 4 : 8, AHEAD = PIPE ? 3 : 6; // (PIPE: the transform's eight patch quads want the registers)
    f32x4 fa[RING];
    auto aload = [&](int slot, int s) { fa[slot] = *reinterpret_cast<const f32x4*>(wp + (long)min(s, nsteps - 1) * step_stride); };

    f32x4 acc[16][NC]; // [position][column tile: tile rows 0 - 3 | 4 - 7 of the block]
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int nc = 0; nc < NC; ++nc)
            acc[i][nc] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    const int btile = lane & 15, kq = lane >> 4;
    const unsigned char* const vsrc = PIPE ? vb + btile * 64 + ((kq ^ ((4 - (btile >> 2)) & 3)) * 16) : vb + btile * VP + kq * 16;
    constexpr int BPOS = PIPE ? G::PVPOS : VPOS, BNT = PIPE ? 16 * 64 : 16 * VP; // B fragment strides: position, second column tile

    gload(0);
    if constexpr (PIPE) { // chunk 0's transform is the one that nothing hides
#pragma unroll
        for (int a = 0; a < AHEAD; ++a)
            aload(a, a);
        to_lds();
        gload(1);
        lds_barrier();
        HP_STAMP();
        transform();
        lds_barrier(); // V[0] is complete and every wavefront has left the patch
        to_lds();      // chunk 1's patch
        gload(2);
        lds_barrier(); // chunk 1's patch is complete
        HP_STAMP();
    } else {
#pragma unroll
        for (int a = 0; a < AHEAD; ++a)
            aload(a, a);
    }
    int s = 0;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        if constexpr (!PIPE) {
            to_lds();      // chunk c's patch (the previous chunk's transform is behind every wavefront: its second barrier)
            gload(c + 1);  // (past the last chunk: a harmless re-read of it)
            lds_barrier(); // the patch is complete AND every wavefront has left the previous chunk's MFMAs: V may be overwritten
            HP_STAMP();
            transform();
            lds_barrier();
            HP_STAMP();
        }
        const unsigned char* const vcur = vsrc + (PIPE ? (c & 1) * G::PVBUF : 0);
        f32x4 fb[2][NC];
#pragma unroll
        for (int nc = 0; nc < NC; ++nc)
            fb[0][nc] = *reinterpret_cast<const f32x4*>(vcur + nc * BNT);
#pragma unroll
        for (int pos = 0; pos < 16; ++pos) {
            const int cur = pos & 1, npos = pos + 1 < 16 ? pos + 1 : pos;
#pragma unroll
            for (int nc = 0; nc < NC; ++nc)
                fb[cur ^ 1][nc] = *reinterpret_cast<const f32x4*>(vcur + npos * BPOS + nc * BNT);
            aload((pos + AHEAD) % RING, s + AHEAD); // (16 % RING == 0: the ring position is a compile-time function of pos)
            const int slot = pos % RING;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nc = 0; nc < NC; ++nc)
                    acc[pos][nc] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[slot][e], fb[cur][nc][e], acc[pos][nc], 0, 0, 0);
            if constexpr (PIPE)
                transform_piece(pos, (c + 1) & 1); // chunk c + 1's transform, one piece per step, under this step's MFMAs
            // issue order of a step: MFMA, LDS read, MFMA, LDS read (the next position's B), MFMA, L2 read (A some steps ahead), 5 MFMAs
            // (the transform's piece - two LDS reads, or a few additions and one LDS write - goes wherever hipcc finds room between them)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if constexpr (NC == 2) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NC == 2 ? 5 : 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            ++s;
        }
        HP_STAMP();
        if constexpr (PIPE) { // the hand-over of chunk c + 2's patch (chunk c + 1's is in LDS, transformed under the steps above)
            if (c + 1 < nch) {
                lds_barrier(); // V[(c + 1) & 1] is complete and every wavefront has left the patch (transform c + 1) and V[c & 1] (chunk c's MFMAs)
                to_lds();
                gload(c + 3); // (past the last chunk: a harmless re-read of it)
                lds_barrier(); // the patch is complete
                HP_STAMP();
            }
        }
    }

    // ---- output transform Y = At M A, per lane: tile 16 nt + (lane & 15), channels 16 wave + 4 kq + r; then whole pixel rows through the
    // block's slab.  Slab row (a * 2 + bb) * 32 + tile = output pixel (2 tile_y + a, 2 tile_x + bb) of the block's 16 x 8
    // The epilogue's inputs first (the ring, the B fragments, the transform's quads and the stage set are dead: their registers hold these
    // now): wavefront w drains slab rows RPW w .. in NPASS passes of RPP pixel rows, lane (row, c4) = channels 4 c4 .. of its row.  Bias, slopes
    // and the residual quads of ALL passes are requested here, so that the output transform and the slab exchange run under those loads.
    int tid_o = tid;
    asm volatile("" : "+v"(tid_o)); // (the lane's coordinates once more from the thread id: kept across the K loop they cost it registers)
    const int lane_o = tid_o & 63, btile_o = lane_o & 15, kq_o = lane_o >> 4;
    using R = rows_geom<G::TMS>;
    constexpr int RPW = 64 * NC / MW, NPASS = RPW / R::RPP;
    static_assert(RPW % R::RPP == 0, "slab rows per pass");
    const int dc4 = lane_o % R::LPR, dm = by * 16 * MW + dc4 * 4;
    // No branch depends on the lane between the first request and the last (a divergent branch is a join at which hipcc waits for every load
    // in flight): clamped addresses instead, every lane loads, the quad path where Cout is whole quads (then a lane's quad is all or nothing)
    const bool dany = dm < p.Cout, quads = (p.Cout & 3) == 0;
    const bool out_vec = quads && ((p.out.coff | p.out.cs) & 3) == 0, res_vec = quads && ((p.res.coff | p.res.cs) & 3) == 0;
    const int dmc = dany ? dm : 0;
    int dpix[NPASS], rpix[NPASS]; // the pixel's index in p.out / p.res (images of t.img pixels, rows of t.wp)
    bool dok[NPASS];
#pragma unroll
    for (int k = 0; k < NPASS; ++k) {
        const int rr = wave * RPW + k * R::RPP + lane_o / R::LPR, ab = rr / (16 * NC), tile = rr % (16 * NC), tr = tile >> 2;
        const int ox = x0 + 2 * (tile & 3) + (ab & 1);
        int oy, ob;
        if (T) // rows form: the block's tile row tr = tile row l0 + tr of image img0, or tr - kb of the next one
            ob = tr >= kb ? img0 + 1 : img0, oy = 2 * (tr >= kb ? tr - kb : l0 + tr) + (ab >> 1);
        else { // tall form: row oy of the batch = row oy % vh of image oy / vh
            oy = y0 + 2 * tr + (ab >> 1);
            ob = vh ? oy / vh : b, oy -= vh ? ob * vh : 0;
        }
        dok[k] = oy < p.OH && ox < p.OW && ob < p.B && dany;
        const int oyc = min(oy, p.OH - 1), oxc = min(ox, p.OW - 1), obc = min(ob, p.B - 1);
        dpix[k] = (obc * p.out.img + oyc * p.out.wp) + oxc;
        rpix[k] = (obc * p.res.img + oyc * p.res.wp) + oxc;
    }
    f32x4 dres[NPASS];
#pragma unroll
    for (int k = 0; k < NPASS; ++k)
        dres[k] = f32x4{ 0.f, 0.f, 0.f, 0.f };
    // (global_load, not flat_load: a flat request counts as LDS traffic too, which the barriers below wait for)
    const gfloat* const gres = (const gfloat*)p.res.p;
    gfloat* const gout = (gfloat*)p.out.p;
    if (gres) {
        if (res_vec) {
#pragma unroll
            for (int k = 0; k < NPASS; ++k)
                dres[k] = *reinterpret_cast<const gf32x4*>(gres + ((long)rpix[k] * p.res.cs + p.res.coff + dmc));
        } else {
#pragma unroll
            for (int k = 0; k < NPASS; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) // (channels past Cout: a re-read of the last one, never stored)
                    dres[k][e] = gres[(long)rpix[k] * p.res.cs + p.res.coff + min(dm + e, p.Cout - 1)];
        }
    }
    // (dm + 3 < Cout_pad: dm is a multiple of 4 below the padded channel count, which is a multiple of 64)
    const f32x4 dbs = *(const gf32x4*)(p.bias + dm);
    f32x4 dsl = { p.act_slope, p.act_slope, p.act_slope, p.act_slope };
    if (p.alpha)
        dsl = *(const gf32x4*)(p.alpha + dm);
    lds_barrier(); // every wavefront is done with V, which the slab lies over (MW = 8: and beyond)
    HP_STAMP();
    float* const slab = reinterpret_cast<float*>(vb);
#pragma unroll
    for (int nt = 0; nt < NC; ++nt) {
        f32x4 S[2][4]; // At M: S[0][j] = M0j + M1j + M2j, S[1][j] = M1j - M2j - M3j
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            S[0][j] = acc[j][nt] + acc[4 + j][nt] + acc[8 + j][nt];
            S[1][j] = acc[4 + j][nt] - acc[8 + j][nt] - acc[12 + j][nt];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const f32x4 y0v = S[a][0] + S[a][1] + S[a][2], y1v = S[a][1] - S[a][2] - S[a][3];
            *reinterpret_cast<f32x4*>(slab + ((a * 2 + 0) * (16 * NC) + nt * 16 + btile_o) * SLAB_PITCH + wave * 16 + kq_o * 4) = y0v;
            *reinterpret_cast<f32x4*>(slab + ((a * 2 + 1) * (16 * NC) + nt * 16 + btile_o) * SLAB_PITCH + wave * 16 + kq_o * 4) = y1v;
        }
    }
    HP_STAMP();
    lds_barrier(); // the slab holds all 16 MW channels of the block's 128 pixels; wavefront w stores rows (128 / MW) w ..
    HP_STAMP();
    // the arithmetic of conv32_drain_rows per element (bias, residual before or after the activation, clamp, slope); the stores of all passes
    // back to back
    const float* const wslab = slab + (wave * RPW + lane_o / R::LPR) * SLAB_PITCH + dc4 * 4;
    f32x4 dv[NPASS];
#pragma unroll
    for (int k = 0; k < NPASS; ++k)
        dv[k] = *reinterpret_cast<const f32x4*>(wslab + k * R::RPP * SLAB_PITCH);
#pragma unroll
    for (int k = 0; k < NPASS; ++k) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = dv[k][e] + dbs[e];
            if (p.res.p && p.res_before_act)
                x += dres[k][e];
            x = x > 0.f ? fminf(x, p.act_hi) : x * dsl[e];
            if (p.res.p && !p.res_before_act)
                x += dres[k][e];
            o[e] = x;
        }
        dv[k] = o;
    }
    if (out_vec) {
#pragma unroll
        for (int k = 0; k < NPASS; ++k)
            if (dok[k])
                *reinterpret_cast<gf32x4*>(gout + ((long)dpix[k] * p.out.cs + p.out.coff + dm)) = dv[k];
    } else {
#pragma unroll
        for (int k = 0; k < NPASS; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (dok[k] && dm + e < p.Cout)
                    gout[(long)dpix[k] * p.out.cs + p.out.coff + dm + e] = dv[k][e];
    }
    HP_STAMP();
#undef HP_STAMP
    if (p.dbg && bx == 1 && by == 0 && tid == 0) // slots 119 - 122: the shader clock and the constant 100 MHz clock at the start / end
        p.dbg[121] = __builtin_readcyclecounter(), p.dbg[122] = __builtin_amdgcn_s_memrealtime();
}

// MFMA work of one launch (what the roofline fraction of this kernel is computed from): 16 products per tile and channel pair
double conv32_winograd_flops(const conv32_params& p)
{
    return 2.0 * 16 * (double)p.B * ((p.OH + 1) / 2) * ((p.OW + 1) / 2) * p.Cout * p.Cin;
}

// packed = [9 taps][cout_pad][cin] fp32 (conv32_params::w's layout) -> U = G g Gt in fragment order [chunk][pos][16-row tile][lane][4 floats]
// (16 * cout_pad * cin floats); lane (row, kq) = channels chunk * 16 + 4 kq + {0..3}.  U is formed in double and rounded to fp32 once.
void conv32_winograd_pack(const float* packed, int cout_pad, int cin, float* out)
{
    static const double G[4][3] = { { 1, 0, 0 }, { .5, .5, .5 }, { .5, -.5, .5 }, { 0, 0, 1 } };
    const int nch = cin / WCK, MT = cout_pad / 16;
    std::vector<double> U((size_t)16 * cout_pad * cin);
    for (int m = 0; m < cout_pad; ++m)
        for (int k = 0; k < cin; ++k) {
            double g[3][3], Gg[4][3];
            for (int t = 0; t < 9; ++t)
                g[t / 3][t % 3] = packed[((size_t)t * cout_pad + m) * cin + k];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 3; ++j)
                    Gg[i][j] = G[i][0] * g[0][j] + G[i][1] * g[1][j] + G[i][2] * g[2][j];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j)
                    U[((size_t)(i * 4 + j) * cout_pad + m) * cin + k] = Gg[i][0] * G[j][0] + Gg[i][1] * G[j][1] + Gg[i][2] * G[j][2];
        }
    for (int c = 0; c < nch; ++c)
        for (int pos = 0; pos < 16; ++pos)
            for (int mt = 0; mt < MT; ++mt) {
                float* dst = out + (((size_t)c * 16 + pos) * MT + mt) * 256;
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int m = mt * 16 + (lane & 15), k = c * WCK + (lane >> 4) * 4 + e;
                        dst[lane * 4 + e] = (float)U[((size_t)pos * cout_pad + m) * cin + k];
                    }
            }
}

template <int MW, bool PIPE, int NC = 2>
static hipError_t launch_wino_case(const conv32_params& q, const conv32_choice& c, hipStream_t s)
{
    constexpr int lds = PIPE ? wino_geom<MW, NC>::PLDS_BYTES : wino_geom<MW, NC>::LDS_BYTES;
    static_assert(MW == WINO_MW && PIPE && lds == WINO_LDS[NC], "conv32_pick.hpp sizes the launch");
    static bool granted = false;
    if (lds > 64 * 1024 && !granted) {
        const hipError_t e = hipFuncSetAttribute((const void*)conv32_winograd_kernel<MW, PIPE, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess)
            return e;
        granted = true;
    }
    HP_LAUNCH((conv32_winograd_kernel<MW, PIPE, NC>), dim3(c.grid_x), dim3(c.threads), lds, s, q, c.tiles_x, c.tiles_y, c.vh, c.rows);
    return hipGetLastError();
}

// Column tiles per block, the per-image / tall / rows form and the grid: pick_conv32 (conv32_pick.hpp)
hipError_t launch_conv32_winograd(const conv32_params& p, const engine_switches& sw, hipStream_t s)
{
    const conv32_choice c = pick_conv32(p, sw, C32_WINO2, false);
    if (!c.ok || !p.w_wino || p.npix <= 0)
        return hipErrorInvalidValue;
#define HP_WINO_CASE(MW_, PIPE_, NC_) \
    if (c.targ[2] == NC_)             \
        return launch_wino_case<MW_, PIPE_, NC_>(p, c, s);
    HP_CONV32_WINO_INSTANCES(HP_WINO_CASE)
#undef HP_WINO_CASE
    return hipErrorInvalidValue;
}

hipError_t conv32_winograd_occupancy(const conv32_params&, int* blocks_per_cu)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, conv32_winograd_kernel<4, true>, 256, wino_geom<4>::PLDS_BYTES);
}

} // namespace hp
