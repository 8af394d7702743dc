// engine.hip -- gfx950 kernels + C ABI for the batched Battlesnake engine.
//
// A lane group owns one game (or one observation) for the duration of a kernel: the game's HBM record (common.h) is
// streamed into LDS with 16-byte loads, the rules are evaluated with one lane per snake, body occupancy is rebuilt in LDS
// from the rings, and the record is streamed back.  The tick: k_step_quad -- a quad per game, sixteen games per wavefront,
// cross-snake questions as DPP quad_perm moves, occupancy as bit planes -- for up to 4 snakes on up to 255 cells; k_step --
// 16 or 64 lanes per game, group-confined shuffles / ballots, byte planes -- for everything else.  All lanes of a group sit
// in one wavefront, so the phases of a kernel are ordered by GAME_SYNC (no workgroup barrier).
// Reference semantics: Game.tic game.py:87-205, Game.make_state game.py:215-257,
// Game.__init__ game.py:13-61, Game.subgame game.py:266-276 (see the per-kernel comments).
#include "common.h"
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void snk_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *snk_last_error(void) { return g_err; }
extern "C" int snk_version(void) { return SNK_ABI_VERSION; }

#define WAVES_PER_BLOCK 4
#define BLOCK_THREADS (WAVES_PER_BLOCK * 64)

// Kernels are templated on the board side: 11x11, 7x7 and 19x19 (the BASELINE configs) get compile-time geometry; any
// other square board runs the same code with the geometry read from the Layout: <0, 0> for boards of at most 255 cells
// (8-bit ring entries), <-1, -1> for larger ones (16-bit entries; CellT<(-1) * (-1)> is the primary template).
template <int NC> struct CellT { using type = uint16_t; };
template <> struct CellT<121> { using type = uint8_t; };
template <> struct CellT<49> { using type = uint8_t; };
template <> struct CellT<0> { using type = uint8_t; };
#define BOARD_DIMS(L)                                                                                   \
    const int HH = H > 0 ? H : (L).H, WW = W > 0 ? W : (L).W;                                           \
    const int NC = HH * WW;                                                                             \
    constexpr int MAXFW = H > 0 ? (H * W + 63) / 64 : (SNK_MAX_CELLS + 63) / 64;                        \
    (void)HH; (void)WW; (void)NC; (void)MAXFW;

__device__ static inline bool food_bit(const uint64_t *food, int c) { return (food[c >> 6] >> (c & 63)) & 1ull; }

// DPP row_share:o (gfx90a+): every lane of a 16-lane row reads lane o of its row
__device__ static inline int row_share16(int v, int o)
{
    switch (o & 15) {
    case 0: return __builtin_amdgcn_update_dpp(0, v, 0x150, 0xF, 0xF, true);
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x151, 0xF, 0xF, true);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0x152, 0xF, 0xF, true);
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x153, 0xF, 0xF, true);
    case 4: return __builtin_amdgcn_update_dpp(0, v, 0x154, 0xF, 0xF, true);
    case 5: return __builtin_amdgcn_update_dpp(0, v, 0x155, 0xF, 0xF, true);
    case 6: return __builtin_amdgcn_update_dpp(0, v, 0x156, 0xF, 0xF, true);
    case 7: return __builtin_amdgcn_update_dpp(0, v, 0x157, 0xF, 0xF, true);
    default: return v;
    }
}

// A game's lanes all sit in ONE wavefront and its LDS region is touched by no other wave, so the phases of a kernel need
// no workgroup barrier: LDS instructions of one wave execute in issue order; what is needed is that the compiler keeps
// them in program order across the phase boundary (a wavefront-scope fence + the wave barrier, which emit no s_barrier).
#define GAME_SYNC()                                                                                     \
    do {                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                          \
        __builtin_amdgcn_wave_barrier();                                                                \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                          \
    } while (0)

// per-wave LDS carve-up used by step / observe
__host__ __device__ static inline int lds_per_wave(const Layout &L) { return L.stride + 4 * L.nc_pad + 64; }
// k_observe: the record + two float planes (channel 0 and channel 1 values per board cell).  Boards of more than 255 cells (16-bit
// ring entries: 19x19 / 8 snakes = 8 KB of rings per record) keep the rings in HBM / L2 and bring only the record's tail (meta,
// food, counters) and the LIVE ring segments -- at most one node per cell plus the stacked tails -- to LDS (round 6: with the
// whole record an observation took 19.8 KB of LDS, 8 wavefronts per CU; now 11.2 KB, 12): obs_rec_bytes
__host__ __device__ static inline int obs_seg_cap(const Layout &L) { return L.nc_pad + 32; }             // live nodes of all snakes
__host__ __device__ static inline int obs_rec_bytes(const Layout &L)
{
    if (L.cell_bytes == 1) return L.stride;
    return (L.stride - L.meta_off) + 32 + (2 * obs_seg_cap(L) + 15) / 16 * 16;       // record tail, 8 segment offsets, the segments
}
__host__ __device__ static inline int lds_per_obs(const Layout &L) { return obs_rec_bytes(L) + 8 * L.nc_pad; }
// k_observe, NHWC planes: + a canvas of the H window rows, 3 (2W-1) H floats (+ two pieces of slack at the ends)
__host__ __device__ static inline int lds_per_wave_win(const Layout &L)
{
    return lds_per_obs(L) + ((3 * (2 * L.W - 1) * L.H + 8) * 4 + 15) / 16 * 16;
}
// k_observe, channel-major planes: + an output canvas of (2H-1)(2W-1)3 floats (+ alignment slack)
__host__ __device__ static inline int lds_per_wave_obs(const Layout &L)
{
    return lds_per_obs(L) + (((2 * L.H - 1) * (2 * L.W - 1) * 3 + 8) * 4 + 15) / 16 * 16;
}

// ------------------------------------------------------------------------------------------
// Game.tic (game.py:87-205)
// GL lanes own one game: 16 (four games per wavefront; 11x11 and 7x7, whose per-game LDS is ~1.2 KB) or 64.  With 4 snakes
// and 121 cells most of a 64-lane wave idles in the per-snake and per-cell steps, and the kernel is instruction-issue
// bound, not HBM bound: four games per wave cut the wave-instructions per game about three times.
// Sub-lane sl = lane % GL plays the role the lane index had; shuffles and ballots are confined to the game's lane group.
// ------------------------------------------------------------------------------------------
template <int H, int W, int GL, int SS = 0>      // SS: compile-time snake count (0 = read it from the layout): the per-snake loops unroll
__global__ __launch_bounds__(BLOCK_THREADS) void k_step(uint8_t *__restrict__ state, Layout L,
                                                       const int32_t *__restrict__ slots, int n,
                                                       const uint8_t *__restrict__ moves,
                                                       const int16_t *__restrict__ spawn_tape,
                                                       uint8_t *__restrict__ done_out,
                                                       int16_t *__restrict__ spawned_out,
                                                       uint64_t *__restrict__ empty_out, int health_dec,
                                                       double chance, uint32_t seed_lo, uint32_t seed_hi,
                                                       const uint8_t *__restrict__ active, const int *__restrict__ skip)
{
    using cell_t = typename CellT<H * W>::type;
    BOARD_DIMS(L)
    constexpr int GPW = 64 / GL;                       // games per wavefront
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sl = lane % GL, gq = lane / GL, gbase = lane - sl;
    const int gi = (blockIdx.x * WAVES_PER_BLOCK + wv) * GPW + gq;
    // games whose `active` flag is 0 are frozen (a rollout sub-game that reached its depth cap, mp_game_runner.py:108):
    // neither loaded nor stored; the flag load is independent of the record load (no slot indirection, one round trip)
    // (skip: the rollout tick's gate, csrc/mcts.hip TICK_GATE -- a non-zero word freezes every game of the launch)
    const bool frozen = gi < n && ((active && !active[gi]) || (skip && *(volatile const int *)skip));
    const bool valid = gi < n && !frozen;
    const int S = SS > 0 ? SS : L.S, mask = L.cap_mask;
// value of sub-lane o of the game's lane group: with 16-lane groups (= one DPP row) a row_share move, one VALU instruction,
// instead of a ds_bpermute through the LDS crossbar (o is a constant after the per-snake loops unroll)
#define GSHFL(v, o) (GL == 16 ? row_share16((v), (o)) : __shfl((v), gbase + (o), 64))
#define GBALLOT(pr) (GL == 64 ? __ballot(pr) : ((__ballot(pr) >> gbase) & ((1ull << (GL & 63)) - 1ull)))
    uint8_t *g = smem + (wv * GPW + gq) * lds_per_wave(L);
    uint8_t *occ = g + L.stride;       // 1 = some snake's non-head node sits here (Game.bodies)
    uint8_t *hd = occ + L.nc_pad;      // 1 = some snake's head sits here (Game.heads, on-board ones)
    const int slot = valid ? (slots ? slots[gi] : gi) : 0;
    uint8_t *gsrc = state + (size_t)slot * L.stride;

    // the per-game inputs do not depend on the record: request them together with it (one HBM round trip, not two)
    const int mv_in = (valid && sl < S) ? moves[(size_t)gi * S + sl] : 1;
    const int tape_in = (valid && spawn_tape) ? spawn_tape[gi] : -1;
    if (valid)
        for (int i = sl; i < L.stride / 16; i += GL) ((uint4 *)g)[i] = ((const uint4 *)gsrc)[i];
    for (int i = sl * 16; i < 2 * L.nc_pad; i += GL * 16) *(uint4 *)(occ + i) = make_uint4(0u, 0u, 0u, 0u);   // both byte planes
    GAME_SYNC();

    SnakeMeta *meta = (SnakeMeta *)(g + L.meta_off);
    uint64_t *food = (uint64_t *)(g + L.food_off);
    uint32_t *cnt = (uint32_t *)(g + L.cnt_off);
    int8_t *rew = (int8_t *)(g + L.rew_off);

    const bool act = valid && sl < S;
    SnakeMeta m = {0, 0, 0, 0, 0};
    if (act) m = meta[sl];
    const bool alive0 = act && m.alive;
    const int n_alive0 = __popcll(GBALLOT(alive0));
    const bool ended = !valid || n_alive0 <= 1;     // tic already returned the rewards list earlier
    const bool go = alive0 && !ended;
    cell_t *ring = (cell_t *)(g + (sl < S ? sl : 0) * L.ring_bytes);

    // ---- execute moves (game.py:90-114; Snake.move game.py:329-358) + health (117-118)
    int head_cell = -1;
    bool oob = false;
    if (go) {
        const int d = (mv_in + m.dir + 3) & 3;            // (move + last - 1) % 4
        m.dir = (uint8_t)d;
        const int hi = (m.tail + m.len - 1) & mask;
        const int hc = ring[hi];
        int y = hc / WW, x = hc - y * WW;
        y += (d == 2) - (d == 0);
        x += (d == 1) - (d == 3);
        oob = (y < 0) | (y >= HH) | (x < 0) | (x >= WW);
        head_cell = oob ? -1 : y * WW + x;
        m.tail = (uint16_t)((m.tail + 1) & mask);      // pop the tail node, push the new head
        if (!oob) ring[(hi + 1) & mask] = (cell_t)head_cell;
        m.health = (int16_t)(m.health - health_dec);
    }
    // ---- food (game.py:121-127): list order, the first snake on a cell eats; Snake.grow (360-365)
    const bool hasfood = go && !oob && food_bit(food, head_cell);
    bool eats = hasfood;
#pragma unroll
    for (int o = 0; o < (SS > 0 ? SS : SNK_MAX_SNAKES); ++o) {
        if (o >= S) break;
        const int ho = GSHFL(head_cell, o);
        const int fo = GSHFL((int)hasfood, o);
        if (o < sl && fo && ho == head_cell) eats = false;
    }
    if (eats) {
        m.health = 100;
        const int t = (m.tail - 1) & mask;
        ring[t] = ring[m.tail];                        // duplicate the tail node
        m.tail = (uint16_t)t;
        m.len = (uint16_t)(m.len + 1);
    }
    const int n_eat = __popcll(GBALLOT(eats));
#pragma unroll
    for (int o = 0; o < (SS > 0 ? SS : SNK_MAX_SNAKES); ++o) {
        if (o >= S) break;
        const int eo = GSHFL((int)eats, o);
        const int co = GSHFL(head_cell, o);
        if (eo && sl == 0) food[co >> 6] &= ~(1ull << (co & 63));
    }
    GAME_SYNC();

    // ---- Game.bodies / Game.heads as LDS byte planes, rebuilt from the rings by all lanes of the game
#pragma unroll
    for (int s = 0; s < (SS > 0 ? SS : SNK_MAX_SNAKES); ++s) {
        if (s >= S) break;
        const int len_s = GSHFL((int)m.len, s);
        const int tail_s = GSHFL((int)m.tail, s);
        const int go_s = GSHFL((int)go, s);
        if (go_s) {
            const cell_t *r = (const cell_t *)(g + s * L.ring_bytes);
            for (int k = sl; k < len_s - 1; k += GL) occ[r[(tail_s + k) & mask]] = 1;
        }
    }
    if (go && !oob) hd[head_cell] = 1;
    GAME_SYNC();

    // ---- spawn food (game.py:130-138).  The game's empty-cell mask is assembled 64 cells per word from GL-cell ballots.
    int spawn = -1;
    if (chance > 0.0 && !ended) {
        int n_food = 0;
        for (int w = 0; w < L.FW; ++w) n_food += __popcll(food[w]);
        uint64_t emk[MAXFW];
        int n_empty = 0;
#pragma unroll
        for (int w = 0; w < MAXFW; ++w) {
            if (w >= L.FW) { emk[w] = 0ull; continue; }
            uint64_t mk = 0ull;
#pragma unroll
            for (int q = 0; q < GPW; ++q) {
                const int c = w * 64 + q * GL + sl;
                const bool e = c < NC && !occ[c] && !hd[c] && !food_bit(food, c);
                mk |= GBALLOT(e) << (q * GL);
            }
            emk[w] = mk;
            if (empty_out && sl == 0) empty_out[(size_t)gi * L.FW + w] = mk;
            n_empty += __popcll(mk);
        }
        if (spawn_tape) {
            spawn = tape_in;
        } else {
            const uint32_t uid = *(const uint32_t *)(g + L.uid_off);
            uint32_t r[4];
            philox4x32(uid, cnt[5], 0x5350574Eu /* 'SPWN' */, 0u, seed_lo, seed_hi, r);
            const double u1 = ((double)r[0] + 0.5) * (1.0 / 4294967296.0);
            if ((n_food == 0 || u1 <= chance) && n_empty > 0) {
                int k = (int)(((uint64_t)r[1] * (uint64_t)n_empty) >> 32);   // uniform in [0, n_empty)
#pragma unroll
                for (int w = 0; w < MAXFW; ++w) {
                    const uint64_t mk = emk[w];
                    const int pc = __popcll(mk);
                    if (spawn < 0) {
                        if (k < pc) {                  // position of the k-th set bit of mk by halving
                            uint64_t t = mk;
                            int pos = 0;
#pragma unroll
                            for (int sh = 32; sh >= 1; sh >>= 1) {
                                const int cl = __popcll(t & ((1ull << sh) - 1ull));
                                if (k >= cl) { k -= cl; t >>= sh; pos += sh; }
                            }
                            spawn = w * 64 + pos;
                        } else {
                            k -= pc;
                        }
                    }
                }
            }
        }
    } else if (empty_out && valid && sl == 0) {
        for (int w = 0; w < L.FW; ++w) empty_out[(size_t)gi * L.FW + w] = 0ull;
    }
    if (spawned_out && valid && sl == 0) spawned_out[gi] = (int16_t)spawn;

    // ---- deaths (game.py:144-165, an if/elif chain) and removal (167-192)
    const bool body_hit = go && !oob && occ[head_cell];
    bool shared = false, lose = false;
#pragma unroll
    for (int o = 0; o < (SS > 0 ? SS : SNK_MAX_SNAKES); ++o) {
        if (o >= S) break;
        const int ho = GSHFL(head_cell, o);
        const int lo = GSHFL((int)m.len, o);
        if (o != sl && ho >= 0 && ho == head_cell) {
            shared = true;
            if ((int)m.len <= lo) lose = true;
        }
    }
    int cause = -1;
    if (go) {
        if (oob) cause = 0;
        else if (body_hit) cause = 1;
        else if (shared) { if (lose) cause = 2; }      // a head-on survivor skips the starvation test
        else if (m.health <= 0) cause = 3;
    }
    const bool dead = cause >= 0;
    const int c0 = __popcll(GBALLOT(cause == 0)), c1 = __popcll(GBALLOT(cause == 1));
    const int c2 = __popcll(GBALLOT(cause == 2)), c3 = __popcll(GBALLOT(cause == 3));
    const int n_alive = __popcll(GBALLOT(go && !dead));
    if (!ended) {
        if (spawn >= 0 && sl == 0) food[spawn >> 6] |= 1ull << (spawn & 63);
        if (dead) {
            m.alive = 0; m.len = 0; m.health = 0; m.dir = 0; m.tail = 0;
            rew[sl] = -1;
        } else if (go && n_alive == 1) {
            rew[sl] = 1;                               // game.py:199-202
        }
        if (act) meta[sl] = m;
        if (sl == 0) {
            cnt[0] += c0; cnt[1] += c1; cnt[2] += c2; cnt[3] += c3;
            cnt[4] += n_eat; cnt[5] += 1;              // game_length (game.py:197)
        }
    }
    GAME_SYNC();
    if (!ended)
        for (int i = sl; i < L.stride / 16; i += GL) ((uint4 *)gsrc)[i] = ((const uint4 *)g)[i];
    if (done_out && valid && sl == 0) done_out[gi] = (uint8_t)(ended || n_alive <= 1);
    if (done_out && frozen && sl == 0) done_out[gi] = 0;
#undef GSHFL
#undef GBALLOT
}

// ------------------------------------------------------------------------------------------
// Game.tic again, for games of at most 4 snakes on boards of at most 255 cells: ONE LANE PER SNAKE, a quad per game,
// sixteen games per wavefront.  k_step above is VALU-issue bound (SQ counters at 262 144 games: 455 VALU instructions
// per wave of four games, three quarters of its lanes idle in the per-snake steps); here every lane of the per-snake steps
// works, cross-snake questions are DPP quad_perm moves (one VALU instruction, no LDS crossbar), the body and head
// occupancy are LDS BIT planes filled with ds_or_b32 by each snake's own lane (its ring walk is sequential), the
// empty-cell mask of the food spawn is three 64-bit logic operations per word, and the death / eat counts of a game
// travel as one packed quad sum.  Same record, same arguments, same results as k_step.
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int q_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
__host__ __device__ constexpr int q_stride(int nc, int s)          // make_layout's stride for 8-bit rings
{
    return (s * q_pow2(nc + 2) + s * 8 + (nc + 63) / 64 * 8 + 24 + (s + 3) / 4 * 4 + 4 + 15) / 16 * 16;
}
__device__ static inline int quad_bcast(int v, int o)              // lane o of the quad
{
    switch (o & 3) {
    case 0: return __builtin_amdgcn_update_dpp(0, v, 0x00, 0xF, 0xF, true);
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x55, 0xF, 0xF, true);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0xAA, 0xF, 0xF, true);
    default: return __builtin_amdgcn_update_dpp(0, v, 0xFF, 0xF, 0xF, true);
    }
}
__device__ static inline int quad_sum(int v)                       // all four lanes get the sum
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    return v;
}
// LDS per game of the quad form: the record + two bit planes (bodies, heads) of QFW 64-bit words each
__host__ __device__ static inline int lds_per_game_quad(const Layout &L) { return L.stride + 16 * ((L.FW + 1) / 2) * 2; }

template <int H, int W, int SS>
__global__ __launch_bounds__(BLOCK_THREADS) void k_step_quad(uint8_t *__restrict__ state, Layout L,
                                                            const int32_t *__restrict__ slots, int n,
                                                            const uint8_t *__restrict__ moves,
                                                            const int16_t *__restrict__ spawn_tape,
                                                            uint8_t *__restrict__ done_out,
                                                            int16_t *__restrict__ spawned_out,
                                                            uint64_t *__restrict__ empty_out, int health_dec,
                                                            double chance, uint32_t seed_lo, uint32_t seed_hi,
                                                            const uint8_t *__restrict__ active, const int *__restrict__ skip)
{
    using cell_t = uint8_t;
    const int HH = H > 0 ? H : L.H, WW = W > 0 ? W : L.W;
    const int NC = HH * WW;
    constexpr int QFW = H > 0 ? (H * W + 63) / 64 : 4;             // 64-bit words of a bit plane (255 cells at most)
    constexpr int CHUNKS = (H > 0 && SS > 0) ? q_stride(H * W, SS) / 16 : 0;
    constexpr int GPWQ = 16;
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sl = lane & 3, gq = lane >> 2;
    const int gi = (blockIdx.x * WAVES_PER_BLOCK + wv) * GPWQ + gq;
    // (skip: the rollout tick's gate, csrc/mcts.hip TICK_GATE -- a non-zero word freezes every game of the launch)
    const bool frozen = gi < n && ((active && !active[gi]) || (skip && *(volatile const int *)skip));
    const bool valid = gi < n && !frozen;
    const int S = SS > 0 ? SS : L.S, mask = L.cap_mask;
    const int FW = H > 0 ? QFW : L.FW;
    const int plane_bytes = 8 * ((L.FW + 1) / 2) * 2;
    uint8_t *g = smem + (size_t)(wv * GPWQ + gq) * L.stride;                       // records first: 16-byte chunks stay aligned
    uint32_t *bodies = (uint32_t *)(smem + (size_t)WAVES_PER_BLOCK * GPWQ * L.stride
                                    + (size_t)(wv * GPWQ + gq) * 2 * plane_bytes);
    uint32_t *heads = bodies + plane_bytes / 4;
    const int slot = valid ? (slots ? slots[gi] : gi) : 0;
    uint8_t *gsrc = state + (size_t)slot * L.stride;

    const int mv_in = (valid && sl < S) ? moves[(size_t)gi * S + sl] : 1;
    const int tape_in = (valid && spawn_tape) ? spawn_tape[gi] : -1;
    if (CHUNKS > 0) {                                              // all loads of the record in flight at once
        uint4 t[(CHUNKS + 3) / 4 > 0 ? (CHUNKS + 3) / 4 : 1];         // unconditional loads (an idle quad re-reads slot 0's
#pragma unroll                                                       // first chunk), so that the array stays in registers
        for (int j = 0; j < (CHUNKS + 3) / 4; ++j)
            t[j] = ((const uint4 *)gsrc)[valid ? min(sl + 4 * j, CHUNKS - 1) : 0];
#pragma unroll
        for (int j = 0; j < (CHUNKS + 3) / 4; ++j)
            if (valid && sl + 4 * j < CHUNKS) ((uint4 *)g)[sl + 4 * j] = t[j];
    } else if (valid) {
        for (int i = sl; i < L.stride / 16; i += 4) ((uint4 *)g)[i] = ((const uint4 *)gsrc)[i];
    }
    for (int i = sl; i < plane_bytes / 2; i += 4) bodies[i] = 0u;                 // both planes
    GAME_SYNC();

    SnakeMeta *meta = (SnakeMeta *)(g + L.meta_off);
    uint64_t *food = (uint64_t *)(g + L.food_off);
    uint32_t *food32 = (uint32_t *)(g + L.food_off);
    uint32_t *cnt = (uint32_t *)(g + L.cnt_off);
    int8_t *rew = (int8_t *)(g + L.rew_off);

    const bool act = valid && sl < S;
    SnakeMeta m = {0, 0, 0, 0, 0};
    if (act) m = meta[sl];
    const bool alive0 = act && m.alive;
    const int n_alive0 = quad_sum((int)alive0);
    const bool ended = !valid || n_alive0 <= 1;
    const bool go = alive0 && !ended;
    cell_t *ring = (cell_t *)(g + (sl < S ? sl : 0) * L.ring_bytes);

    // ---- execute moves (game.py:90-114) + health (117-118)
    int head_cell = -1;
    bool oob = false;
    if (go) {
        const int d = (mv_in + m.dir + 3) & 3;
        m.dir = (uint8_t)d;
        const int hi = (m.tail + m.len - 1) & mask;
        const int hc = ring[hi];
        int y = hc / WW, x = hc - y * WW;
        y += (d == 2) - (d == 0);
        x += (d == 1) - (d == 3);
        oob = (y < 0) | (y >= HH) | (x < 0) | (x >= WW);
        head_cell = oob ? -1 : y * WW + x;
        m.tail = (uint16_t)((m.tail + 1) & mask);
        if (!oob) ring[(hi + 1) & mask] = (cell_t)head_cell;
        m.health = (int16_t)(m.health - health_dec);
    }
    // ---- food (game.py:121-127): the first snake in list order on a cell eats
    const bool hasfood = go && !oob && ((food32[head_cell >> 5] >> (head_cell & 31)) & 1u);
    bool eats = hasfood;
    const int fcell = hasfood ? head_cell : -1;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const int fo = quad_bcast(fcell, o);
        if (o < sl && fo >= 0 && fo == head_cell) eats = false;
    }
    if (eats) {
        m.health = 100;
        const int t = (m.tail - 1) & mask;
        ring[t] = ring[m.tail];                        // duplicate the tail node (Snake.grow game.py:360-365)
        m.tail = (uint16_t)t;
        m.len = (uint16_t)(m.len + 1);
        atomicAnd(&food32[head_cell >> 5], ~(1u << (head_cell & 31)));
    }
    // ---- Game.bodies / Game.heads as bit planes: every snake's own lane walks its ring
    if (go) {
        for (int k = 0; k < (int)m.len - 1; ++k) {
            const int c = ring[(m.tail + k) & mask];
            atomicOr(&bodies[c >> 5], 1u << (c & 31));
        }
        if (!oob) atomicOr(&heads[head_cell >> 5], 1u << (head_cell & 31));
    }
    GAME_SYNC();

    // ---- spawn food (game.py:130-138): empty = not body, not head, not food
    int spawn = -1;
    if (chance > 0.0 && !ended) {
        int n_food = 0, n_empty = 0;
        uint64_t emk[QFW];
#pragma unroll
        for (int w = 0; w < QFW; ++w) {
            emk[w] = 0ull;
            if (w < FW) {
                const uint64_t fw = food[w];
                const uint64_t used = fw | ((const uint64_t *)bodies)[w] | ((const uint64_t *)heads)[w];
                const int left = NC - 64 * w;                                       // cells of this word
                const uint64_t cells = left >= 64 ? ~0ull : ((1ull << (left > 0 ? left : 0)) - 1ull);
                emk[w] = ~used & cells;
                n_food += __popcll(fw);
                n_empty += __popcll(emk[w]);
                if (empty_out && sl == 0) empty_out[(size_t)gi * L.FW + w] = emk[w];
            }
        }
        if (spawn_tape) {
            spawn = tape_in;
        } else {
            const uint32_t uid = *(const uint32_t *)(g + L.uid_off);
            uint32_t r[4];
            philox4x32(uid, cnt[5], 0x5350574Eu /* 'SPWN' */, 0u, seed_lo, seed_hi, r);
            const double u1 = ((double)r[0] + 0.5) * (1.0 / 4294967296.0);
            if ((n_food == 0 || u1 <= chance) && n_empty > 0) {
                int k = (int)(((uint64_t)r[1] * (uint64_t)n_empty) >> 32);
#pragma unroll
                for (int w = 0; w < QFW; ++w) {
                    const uint64_t mk = emk[w];
                    const int pc = __popcll(mk);
                    if (spawn < 0) {
                        if (k < pc) {
                            uint64_t t = mk;
                            int pos = 0;
#pragma unroll
                            for (int sh = 32; sh >= 1; sh >>= 1) {
                                const int cl = __popcll(t & ((1ull << sh) - 1ull));
                                if (k >= cl) { k -= cl; t >>= sh; pos += sh; }
                            }
                            spawn = w * 64 + pos;
                        } else {
                            k -= pc;
                        }
                    }
                }
            }
        }
    } else if (empty_out && valid && sl == 0) {
        for (int w = 0; w < L.FW; ++w) empty_out[(size_t)gi * L.FW + w] = 0ull;
    }
    if (spawned_out && valid && sl == 0) spawned_out[gi] = (int16_t)spawn;

    // ---- deaths (game.py:144-165) and removal (167-192)
    const bool body_hit = go && !oob && ((bodies[head_cell >> 5] >> (head_cell & 31)) & 1u);
    bool shared = false, lose = false;
    const int hl = (head_cell + 1) | ((int)m.len << 9);            // head_cell + 1 <= 255, length in the bits above
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int q = quad_bcast(hl, o);
        const int ho = (q & 511) - 1, lo = q >> 9;
        if (o != sl && ho >= 0 && ho == head_cell) {
            shared = true;
            if ((int)m.len <= lo) lose = true;
        }
    }
    int cause = -1;
    if (go) {
        if (oob) cause = 0;
        else if (body_hit) cause = 1;
        else if (shared) { if (lose) cause = 2; }
        else if (m.health <= 0) cause = 3;
    }
    const bool dead = cause >= 0;
    const int tally = quad_sum((cause >= 0 ? 1 << (3 * cause) : 0) | ((go && !dead) ? 1 << 12 : 0) | (eats ? 1 << 15 : 0));
    const int n_alive = (tally >> 12) & 7;
    if (!ended) {
        if (dead) {
            m.alive = 0; m.len = 0; m.health = 0; m.dir = 0; m.tail = 0;
            rew[sl] = -1;
        } else if (go && n_alive == 1) {
            rew[sl] = 1;
        }
        if (act) meta[sl] = m;
        if (sl == 0) {
            if (spawn >= 0) food[spawn >> 6] |= 1ull << (spawn & 63);
            cnt[0] += tally & 7; cnt[1] += (tally >> 3) & 7; cnt[2] += (tally >> 6) & 7; cnt[3] += (tally >> 9) & 7;
            cnt[4] += (tally >> 15) & 7; cnt[5] += 1;
        }
    }
    GAME_SYNC();
    if (!ended) {
        if (CHUNKS > 0) {
#pragma unroll
            for (int j = 0; j < (CHUNKS + 3) / 4; ++j)
                if (sl + 4 * j < CHUNKS) ((uint4 *)gsrc)[sl + 4 * j] = ((const uint4 *)g)[sl + 4 * j];
        } else {
            for (int i = sl; i < L.stride / 16; i += 4) ((uint4 *)gsrc)[i] = ((const uint4 *)g)[i];
        }
    }
    if (done_out && valid && sl == 0) done_out[gi] = (uint8_t)(ended || n_alive <= 1);
    if (done_out && frozen && sl == 0) done_out[gi] = 0;
}

// ------------------------------------------------------------------------------------------
// Game.__init__ (game.py:13-61)
// ------------------------------------------------------------------------------------------
template <int H, int W>
__global__ __launch_bounds__(BLOCK_THREADS) void k_reset(uint8_t *__restrict__ state, Layout L,
                                                        const int32_t *__restrict__ slots, int n,
                                                        const uint8_t *__restrict__ tape, uint32_t uid_base,
                                                        uint32_t seed_lo, uint32_t seed_hi)
{
    using cell_t = typename CellT<H * W>::type;
    BOARD_DIMS(L)
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int gi = blockIdx.x * WAVES_PER_BLOCK + wv;
    const bool valid = gi < n;
    const int S = L.S;
    uint8_t *g = smem + wv * lds_per_wave(L);
    for (int i = lane; i < L.stride / 16; i += 64) ((uint4 *)g)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (valid && lane == 0) {
        const int sy[8] = {1, HH - 2, HH - 2, 1, 1, HH / 2, HH - 2, HH / 2};
        const int sx[8] = {1, WW - 2, 1, WW - 2, WW / 2, WW - 2, WW / 2, 1};
        uint8_t pos[8], dirs[8], fc[8];
        const uint32_t uid = uid_base + (uint32_t)gi;
        if (tape) {
            for (int s = 0; s < S; ++s) {
                pos[s] = tape[((size_t)gi * 3 + 0) * S + s];
                dirs[s] = tape[((size_t)gi * 3 + 1) * S + s];
                fc[s] = tape[((size_t)gi * 3 + 2) * S + s];
            }
        } else {
            uint32_t r[24];
            for (int q = 0; q < 6; ++q) philox4x32(uid, (uint32_t)q, 0x494E4954u /* 'INIT' */, 0u, seed_lo, seed_hi, r + 4 * q);
            uint8_t perm[8] = {0, 1, 2, 3, 4, 5, 6, 7};
            for (int s = 0; s < S; ++s) {          // random.sample(8 start cells, S): ordered S-subset
                const int j = s + (int)(((uint64_t)r[s] * (uint64_t)(8 - s)) >> 32);
                const uint8_t t = perm[s]; perm[s] = perm[j]; perm[j] = t;
                pos[s] = perm[s];
                dirs[s] = (uint8_t)(r[8 + s] >> 30);
                fc[s] = (uint8_t)(r[16 + s] >> 30);
            }
        }
        SnakeMeta *meta = (SnakeMeta *)(g + L.meta_off);
        uint64_t *food = (uint64_t *)(g + L.food_off);
        const int center = (HH / 2) * WW + WW / 2;
        food[center >> 6] |= 1ull << (center & 63);
        for (int s = 0; s < S; ++s) {
            const int y = sy[pos[s]], x = sx[pos[s]];
            cell_t *ring = (cell_t *)(g + s * L.ring_bytes);
            ring[0] = ring[1] = ring[2] = (cell_t)(y * WW + x);     // 3 stacked nodes (game.py:37)
            meta[s].tail = 0; meta[s].len = 3; meta[s].health = 100; meta[s].dir = dirs[s]; meta[s].alive = 1;
            const int fy = y + ((fc[s] & 2) ? 1 : -1), fx = x + ((fc[s] & 1) ? 1 : -1);
            const int c = fy * WW + fx;
            food[c >> 6] |= 1ull << (c & 63);
        }
        *(uint32_t *)(g + L.uid_off) = uid;
    }
    __syncthreads();
    if (valid) {
        const int slot = slots ? slots[gi] : gi;
        uint8_t *gdst = state + (size_t)slot * L.stride;
        for (int i = lane; i < L.stride / 16; i += 64) ((uint4 *)gdst)[i] = ((const uint4 *)g)[i];
    }
}

// ------------------------------------------------------------------------------------------
// Game.subgame (game.py:266-276): one wavefront reads a parent once and writes `fanout` copies
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK_THREADS) void k_clone(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        Layout L, const int32_t *__restrict__ src_slots, int n,
                                                        const int32_t *__restrict__ dst_slots, int fanout)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int gi = blockIdx.x * WAVES_PER_BLOCK + wv;
    if (gi >= n) return;
    const int ss = src_slots ? src_slots[gi] : gi;
    const uint4 *p = (const uint4 *)(src + (size_t)ss * L.stride);
    const int nq = L.stride / 16;
    // the counters (6 x u32 at cnt_off, 8-byte aligned) are zeroed in flight
    const int c_lo = L.cnt_off, c_hi = L.cnt_off + 24;
    for (int i = lane; i < nq; i += 64) {
        uint4 v = p[i];
        uint32_t *w = (uint32_t *)&v;
        for (int q = 0; q < 4; ++q) {
            const int off = i * 16 + q * 4;
            if (off >= c_lo && off < c_hi) w[q] = 0u;
        }
        for (int j = 0; j < fanout; ++j) {
            const int ds = dst_slots ? dst_slots[(size_t)gi * fanout + j] : gi * fanout + j;
            ((uint4 *)(dst + (size_t)ds * L.stride))[i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// alive flags (Game.get_ids, game.py:76-77)
// ------------------------------------------------------------------------------------------
__global__ void k_alive(const uint8_t *__restrict__ state, Layout L, const int32_t *__restrict__ slots, int n,
                        uint8_t *__restrict__ alive_out, int32_t *__restrict__ n_alive_out)
{
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n) return;
    const int slot = slots ? slots[gi] : gi;
    const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)slot * L.stride + L.meta_off);
    int c = 0;
    for (int s = 0; s < L.S; ++s) {
        const uint8_t a = meta[s].alive;
        alive_out[(size_t)gi * L.S + s] = a;
        c += a;
    }
    if (n_alive_out) n_alive_out[gi] = c;
}

__global__ void k_sum_counters(const uint8_t *__restrict__ state, Layout L, const int32_t *__restrict__ slots, int n,
                               unsigned long long *__restrict__ out6)
{
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < n; gi += gridDim.x * blockDim.x) {
        const int slot = slots ? slots[gi] : gi;
        const uint32_t *c = (const uint32_t *)(state + (size_t)slot * L.stride + L.cnt_off);
        for (int q = 0; q < 6; ++q) acc[q] += c[q];
    }
    for (int q = 0; q < 6; ++q) {
        const unsigned long long s = wave_sum_u64(acc[q]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out6[q], s);
    }
}

// ------------------------------------------------------------------------------------------
// Game.make_state (game.py:215-257) + obstacle test (alpha_nnet.py:63-76) + observation key
// GL lanes per (slot, snake) pair: 16 (four observations per wavefront; 11x11 and 7x7) or 64 (19x19).  Everything before
// the first plane byte (record load, tail-distance plane, 2 x splitmix64 per board cell for the key) is per-observation
// work that left most of a 64-lane wave idle; with four observations per wave it costs a quarter of the instructions.
// The host uses GL = 16 for requests without planes and GL = 64 for requests with planes (see snk_engine_observe).
// ------------------------------------------------------------------------------------------
template <int H, int W, int GL, int WPB>
__global__ __launch_bounds__(WPB * 64) void k_observe(const uint8_t *__restrict__ state, Layout L,
                                                          const int32_t *__restrict__ pairs, int m, int layout,
                                                          float *__restrict__ planes, uint8_t *__restrict__ mask_out,
                                                          uint64_t *__restrict__ key_out, int legacy_mask, int reps,
                                                          const int32_t *__restrict__ index, const uint8_t *__restrict__ sub_active,
                                                          uint8_t *__restrict__ row_active, const uint8_t *__restrict__ mirror)
{
    // mirror (optional): mirror[i] != 0 writes row i's planes flipped on the W axis, numpy.flip(states, axis=2) of the trainer's
    // augmentation (trainer.py:93-97): the board cells go to column N-1-j AFTER the rot90 map; the wall background and the centre
    // pixel are symmetric.  Planes only: mask and key of a mirrored row are not defined (snk_engine_observe_mirror passes neither).
    // index (optional): output row i observes pairs[index[i]] (the rollout tick's rows to evaluate: no gathered copy of the pairs);
    // row_active (optional, with sub_active): row_active[i] = the observing snake is alive AND sub_active[its slot] -- the tick's
    // "which rows are live" (mp_game_runner.py:99-103) taken where the record is in hand instead of by two launches of its own
    using cell_t = typename CellT<H * W>::type;
    BOARD_DIMS(L)
    const int N = 2 * HH - 1, NPIX = N * N, NEL = NPIX * 3;
    static_assert(H == W, "only square boards batch (rot90 transposes odd-k shapes)");
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr int GPW = 64 / GL;                       // observations per wavefront
    // wave-uniform values are made scalar (readfirstlane): with a whole wavefront per observation everything derived from
    // the pair, the observing snake's meta word and its head then runs on the scalar unit instead of costing VALU issue
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sl = lane % GL, gq = lane / GL;
    // A lane group takes `reps` consecutive observations, one after the other, the next one's record already travelling
    // while the current one is worked on: a wavefront's life is two dependent loads (pair, record), the work, and the wait
    // for its stores to be acknowledged (s_endpgm waits for them); with one observation per wavefront that chain, not the
    // instruction count or the HBM rate, set the time (measured: 8 192 wave slots x 5.3 KB per ~10 us lifetime).
    const int pi0 = ((blockIdx.x * WPB + wv) * GPW + gq) * reps;
    const int S = L.S, mask = L.cap_mask;
    constexpr bool RG = sizeof(cell_t) == 2;              // rings stay in global memory (lds_per_obs above)
    const int roff = RG ? L.meta_off : 0;                 // first byte of the record that is staged in LDS
    const int nch = (L.stride - roff) / 16;
    uint4 ahead = make_uint4(0u, 0u, 0u, 0u);             // chunk `sl` of the (staged part of the) record of the next observation
    int ahead_you = 0, ahead_slot = 0;
    const uint8_t *ahead_src = state;
    if (pi0 < m) {
        const int pr = index ? index[pi0] : pi0;
        ahead_slot = pairs[2 * pr];
        ahead_src = state + (size_t)ahead_slot * L.stride;
        ahead_you = pairs[2 * pr + 1];
        if (sl < nch) ahead = ((const uint4 *)(ahead_src + roff))[sl];
    }
    for (int rep = 0; rep < reps; ++rep) {
    const int pi = pi0 + rep;
    const bool valid = pi < m;
    const bool mir = mirror && valid && mirror[pi];
    uint8_t *g = smem + (wv * GPW + gq) * (!planes ? lds_per_obs(L) : layout == SNK_NHWC_F32 ? lds_per_wave_win(L) : lds_per_wave_obs(L));
    float *v1 = (float *)(g + obs_rec_bytes(L));            // channel 1 per board cell: 0.02 x the largest tail-distance of a node on it
    float *v0 = v1 + L.nc_pad;                              // channel 0 per board cell: the head value of the snake whose head is here
    int *seg_off = (int *)(g + (L.stride - roff));          // RG: where each snake's live segment starts in `seg`
    cell_t *seg = (cell_t *)(g + (L.stride - roff) + 32);   // RG: the snakes' nodes tail -> head, one snake after the other

    const int you = ahead_you, slot = ahead_slot;
    const uint8_t *gsrc = ahead_src;
    if (valid && sl < nch) ((uint4 *)g)[sl] = ahead;
    if (valid)
        for (int i = sl + GL; i < nch; i += GL) ((uint4 *)g)[i] = ((const uint4 *)(gsrc + roff))[i];
    if (rep + 1 < reps && pi + 1 < m) {                     // request the next record now
        const int pr = index ? index[pi + 1] : pi + 1;
        ahead_slot = pairs[2 * pr];
        ahead_src = state + (size_t)ahead_slot * L.stride;
        ahead_you = pairs[2 * pr + 1];
        if (sl < nch) ahead = ((const uint4 *)(ahead_src + roff))[sl];
    }
    for (int i = sl * 16; i < 8 * L.nc_pad; i += GL * 16) *(uint4 *)((uint8_t *)v1 + i) = make_uint4(0u, 0u, 0u, 0u);   // both planes
    GAME_SYNC();

    const SnakeMeta *meta = (const SnakeMeta *)(g + L.meta_off - roff);
    const uint64_t *food = (const uint64_t *)(g + L.food_off - roff);
    if constexpr (RG) {
        // the live ring segments, straight from the record in global memory (its rings are L2-resident: the snakes of a game share
        // them) into `seg`, all snakes in ONE flattened pass so that the loads of different snakes travel together
        int tl_[SNK_MAX_SNAKES], of_[SNK_MAX_SNAKES], total = 0;
#pragma unroll
        for (int s = 0; s < SNK_MAX_SNAKES; ++s) {
            SnakeMeta ms = meta[s < S ? s : 0];
            const int len = (valid && s < S && ms.alive) ? (int)ms.len : 0;
            tl_[s] = ms.tail; of_[s] = total; total += len;
        }
        total = min(total, obs_seg_cap(L));                 // (a legal board holds at most one node per cell plus the stacked tails)
        if (sl < SNK_MAX_SNAKES) {
            int o = 0;
#pragma unroll
            for (int s = 0; s < SNK_MAX_SNAKES; ++s) o = sl == s ? of_[s] : o;
            seg_off[sl] = o;
        }
        for (int idx = sl; idx < total; idx += GL) {
            int s = 0, tl = tl_[0], of = 0;
#pragma unroll
            for (int q = 1; q < SNK_MAX_SNAKES; ++q)
                if (idx >= of_[q]) { s = q; tl = tl_[q]; of = of_[q]; }     // the LAST snake that starts at or before idx (dead ones are empty)
            seg[idx] = ((const cell_t *)(gsrc + s * L.ring_bytes))[(tl + (idx - of)) & mask];
        }
        GAME_SYNC();
    }
    SnakeMeta me = meta[you];
    if (GL == 64) {
        uint2 w = *(const uint2 *)&me;
        w.x = __builtin_amdgcn_readfirstlane(w.x); w.y = __builtin_amdgcn_readfirstlane(w.y);
        me = *(const SnakeMeta *)&w;
    }
    const bool live = valid && me.alive;

    // body plane: walking tail -> head with dist 1,2,... the last write wins (game.py:236-241);
    // only the node nearest the head of a run of stacked nodes writes, so there is no race.
    // With a whole wavefront per observation and at most four snakes, sixteen lanes walk each snake at once (one pass for
    // bodies of up to 16 nodes) instead of all lanes walking the snakes one after the other.  (Alive snakes never share a
    // cell in a state a tick produced, so the order between snakes does not matter.)
    constexpr int LPS = GL == 64 ? 16 : GL;              // lanes per snake
    const bool by_snake = GL == 64 && S <= 4;
    for (int s0 = 0; s0 < S; ++s0) {
        if (!valid) break;                               // an idle wave holds no record: touch nothing
        const int s = by_snake ? sl / LPS : s0;
        if (by_snake && (s0 > 0 || s >= S)) break;
        const SnakeMeta ms = meta[s];
        if (!ms.alive) continue;
        // node k of snake s, tail -> head: from the ring in LDS, or (RG) from the snake's segment
        const cell_t *r = RG ? seg + seg_off[s] : (const cell_t *)(g + s * L.ring_bytes);
        const int rt = RG ? 0 : ms.tail, rm = RG ? 0xFFFF : mask;
        const int len_s = RG ? min((int)ms.len, obs_seg_cap(L) - seg_off[s]) : (int)ms.len;
        for (int k = by_snake ? sl % LPS : sl; k < len_s; k += LPS) {
            const int c = r[(rt + k) & rm];
            const bool last = (k == ms.len - 1) || (r[(rt + k + 1) & rm] != c);
            if (last) v1[c] = (float)((double)(k + 1) * 0.02);          // float64 product, then float32 (game.py:236-241, 257)
            if (k == ms.len - 1)   // (snake.length - (you.length - 0.5)) * 0.04 in float64, then float32 (game.py:229-232,257)
                v0[c] = (float)(((double)ms.len - ((double)me.len - 0.5)) * 0.04);
        }
    }
    GAME_SYNC();

    int my_head = RG ? (int)seg[max(0, min(seg_off[you] + me.len - 1, obs_seg_cap(L) - 1))]
                     : (int)((const cell_t *)(g + you * L.ring_bytes))[(me.tail + me.len - 1) & mask];
    if (GL == 64) my_head = __builtin_amdgcn_readfirstlane(my_head);
    const int hy = my_head / WW, hx = my_head - hy * WW;
    const int k = me.dir & 3;
    const float fval = (float)((double)(101 - (int)me.health) * 0.01);   // game.py:243-244

    // value of board cell c, channel ch, exactly as make_state writes it
    auto cell_val = [&](int c, int ch) -> float {
        if (c == my_head) return -1.0f;                                   // game.py:248
        if (ch == 0) return v0[c];
        if (ch == 1) return v1[c];
        return food_bit(food, c) ? fval : 0.0f;
    };

    if (planes && layout == SNK_NHWC_F32) {
        // The reference's layout, the one the net reads: every output byte is written once, in aligned 16-byte pieces.
        // The observation is the wall pattern (0, 1, 0 per pixel) except inside the H canvas rows the board window occupies
        // -- one contiguous element range.  Pieces outside that range go out straight from registers (the pattern of a piece
        // depends on the channel of its first element only, which advances by one from a lane's piece to its next: three
        // float4 registers used in turn); pieces inside it are first laid into a small LDS canvas (window rows only), the
        // board cells are scattered over them there, and the canvas is streamed out.  Measured on the way: the full-canvas
        // form with per-element pattern arithmetic was VALU-issue bound (SQ counters: 715 VALU instructions per observation,
        // 104 us of VALU issue against 67 us of HBM time at 78 229 observations); pattern everywhere + cells stored over it
        // as 12-byte pixels cost 50 us for the cells alone (partial-line writes of lines that had left the L2).
        float *out = planes + (size_t)pi * NEL;
        const int lead = (int)(((size_t)pi * NEL) & 3);               // out + e is 16-byte aligned where (e + lead) % 4 == 0
        const int nvec = (NEL + lead + 3) / 4;                          // piece q = elements 4 q - lead .. 4 q - lead + 3
        float *cvs = (float *)(g + lds_per_obs(L));                    // cvs[4 (q - qa) + t] <-> element 4 q - lead + t
        int qa = 0, qb = 0;                                            // pieces of the window rows
        if (live) {
            const int i0 = k == 0 ? HH - 1 - hy : k == 1 ? hx : k == 2 ? hy : WW - 1 - hx;   // first canvas row of the window
            qa = (3 * N * i0 + lead) >> 2;
            qb = (3 * N * (i0 + HH) + lead + 3) >> 2;
        }
        const int q_lo = lead ? 1 : 0, q_hi = (NEL + lead) >> 2;       // pieces q_lo <= q < q_hi lie wholly inside the observation
        const float one = live ? 1.0f : 0.0f;                          // the observation of a dead snake is all zeros
        if (valid) {
            static_assert((4 * GL) % 3 == 1, "the channel of a lane's next piece advances by one");
            const int c0 = (4 * sl - lead + 3) % 3;                    // channel of the first element of piece q = sl
            const float a = c0 == 0 ? one : 0.0f, b = c0 == 1 ? one : 0.0f, c = c0 == 2 ? one : 0.0f;
            float4 p0 = make_float4(b, a, c, b), p1 = make_float4(a, c, b, a), p2 = make_float4(c, b, a, c);
            for (int q = sl; q < nvec; q += GL) {
                if ((unsigned)(q - qa) < (unsigned)(qb - qa)) *(float4 *)(cvs + 4 * (q - qa)) = p0;
                else if ((unsigned)(q - q_lo) < (unsigned)(q_hi - q_lo)) *(float4 *)(out + (4 * q - lead)) = p0;
                const float4 t4 = p0; p0 = p1; p1 = p2; p2 = t4;
            }
        }
        GAME_SYNC();
        if (live) {
            const int base = lead - 4 * qa;
            for (int c = sl; c < NC; c += GL) {
                const int y = c / WW, x = c - y * WW;
                const int si = y - hy + (HH - 1), sj = x - hx + (WW - 1);
                int i, j;                              // numpy.rot90(grid, k): out[i][j] = grid[si][sj], inverted
                if (k == 0) { i = si; j = sj; }
                else if (k == 1) { i = N - 1 - sj; j = si; }
                else if (k == 2) { i = N - 1 - si; j = N - 1 - sj; }
                else { i = sj; j = N - 1 - si; }
                if (mir) j = N - 1 - j;                // (the window rows qa..qb depend on i alone and hold all N columns)
                float *px = cvs + (3 * (i * N + j) + base);
                px[0] = v0[c]; px[1] = v1[c]; px[2] = food_bit(food, c) ? fval : 0.0f;
            }
            // the observer's own head (game.py:248) is the centre pixel whatever the rotation: -1 in all three channels,
            // written after the scatter (LDS instructions of a wave execute in order)
            if (sl < 3) cvs[3 * ((HH - 1) * N + (WW - 1)) + base + sl] = -1.0f;
        }
        GAME_SYNC();
        if (live)
            for (int q = max(qa, q_lo) + sl; q < min(qb, q_hi); q += GL)
                *(float4 *)(out + (4 * q - lead)) = *(const float4 *)(cvs + 4 * (q - qa));
        // the at most 3 + 3 elements of the partial pieces at both ends: lanes 0..3 the head, lanes 4..7 the tail
        if (valid && sl < 8) {
            const int e = sl < 4 ? sl : 4 * q_hi - lead + (sl - 4);
            const bool mine = sl < 4 ? (sl < 4 * q_lo - lead) : (e < NEL);
            if (mine) {
                const int q = (e + lead) >> 2;
                float v = (e % 3 == 1) ? one : 0.0f;
                if ((unsigned)(q - qa) < (unsigned)(qb - qa)) v = cvs[e + lead - 4 * qa];
                out[e] = v;
            }
        }
    } else if (planes) {
        // The channel-major layouts.  The observation is the wall pattern almost everywhere (441 canvas pixels, 121 board cells): fill an LDS
        // canvas with the pattern, scatter the board cells into their rotated positions, stream the canvas out
        // with 16-byte stores.  The canvas is shifted by `lead` floats so that LDS and HBM addresses are congruent
        // mod 16 bytes whatever the row's position in the output array.
        float *out = planes + (size_t)pi * NEL;
        float *canvas = (float *)(g + lds_per_obs(L));
        const int lead = (layout == SNK_NCHW_BF16) ? 0 : (int)(((size_t)pi * NEL) & 3);
        float *cv = canvas + lead;                     // cv[e] <-> out[e]
        const int nvec = (NEL + lead + 3) / 4;
        if (valid)
        {
            // channel (element % 3) of the float4's first element: one division here, then it advances by 4 GL mod 3 per
            // iteration (the per-element `% 3` cost four quarter-rate multiplies per float4)
            int ch0 = (4 * sl - lead + 3) % 3;
            constexpr int ADV = (4 * GL) % 3;
            for (int q = sl; q < nvec; q += GL) {
                float4 v;
                float *pv = (float *)&v;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int e = 4 * q - lead + t;
                    int ch = ch0 + t;                  // 0 .. 5
                    ch -= ch >= 3 ? 3 : 0;
                    float d = 0.0f;
                    if (live) d = (layout == SNK_NHWC_F32) ? ((ch == 1) ? 1.0f : 0.0f)
                                                           : ((e >= NPIX && e < 2 * NPIX) ? 1.0f : 0.0f);   // WALL (game.py:4,219)
                    pv[t] = d;
                }
                *(float4 *)(canvas + 4 * q) = v;
                ch0 += ADV;
                ch0 -= ch0 >= 3 ? 3 : 0;
            }
        }
        GAME_SYNC();
        if (live)
            for (int c = sl; c < NC; c += GL) {
                const int y = c / WW, x = c - y * WW;
                const int si = y - hy + (HH - 1), sj = x - hx + (WW - 1);
                int i, j;                              // numpy.rot90(grid, k): out[i][j] = grid[si][sj], inverted
                if (k == 0) { i = si; j = sj; }
                else if (k == 1) { i = N - 1 - sj; j = si; }
                else if (k == 2) { i = N - 1 - si; j = N - 1 - sj; }
                else { i = sj; j = N - 1 - si; }
                if (mir) j = N - 1 - j;
                const int pp = i * N + j;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    cv[(layout == SNK_NHWC_F32) ? 3 * pp + ch : ch * NPIX + pp] = cell_val(c, ch);
            }
        GAME_SYNC();
        if (valid && layout == SNK_NCHW_BF16) {            // same values, channel-major, rounded to bf16 (nearest even)
            unsigned short *o16 = (unsigned short *)planes + (size_t)pi * NEL;
            for (int e = sl; e < NEL; e += GL) {
                const uint32_t u = __float_as_uint(canvas[e]);
                o16[e] = (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);      // observation values are finite
            }
        } else if (valid)
            for (int q = sl; q < nvec; q += GL) {
                const int e0 = 4 * q - lead;
                const float4 v = *(const float4 *)(canvas + 4 * q);
                if (e0 >= 0 && e0 + 3 < NEL) {
                    *(float4 *)(out + e0) = v;
                } else {
                    const float *pv = (const float *)&v;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (e0 + t >= 0 && e0 + t < NEL) out[e0 + t] = pv[t];
                }
            }
    }
    if (row_active && valid && sl == 0) row_active[pi] = (live && sub_active[slot]) ? 1 : 0;
    if (mask_out && valid && sl < 3) {
        uint8_t b = 1;
        if (live) {
            const int ad = (k + 3 + sl) & 3;           // left / straight / right of the heading
            const int y = hy + (ad == 2) - (ad == 0), x = hx + (ad == 1) - (ad == 3);
            float v = 1.0f;
            if (y >= 0 && y < HH && x >= 0 && x < WW) v = cell_val(y * WW + x, 1);
            b = legacy_mask ? ((double)v >= 0.04) : (v >= 0.04f);          // alpha_nnet.py:75-76
        }
        mask_out[(size_t)pi * 3 + sl] = b;
    }
    if (key_out) {
        uint64_t lo = 0, hi = 0;
        if (live) {
            for (int c = sl; c < NC; c += GL) {
                const uint32_t b0 = __float_as_uint(cell_val(c, 0)), b1 = __float_as_uint(cell_val(c, 1)),
                               b2 = __float_as_uint(cell_val(c, 2));
                if (b0 == 0u && b1 == 0x3F800000u && b2 == 0u) continue;   // indistinguishable from a wall
                const int y = c / WW, x = c - y * WW;
                const int si = y - hy + (HH - 1), sj = x - hx + (WW - 1);
                int i, j;                                // inverse of the rot90 map above
                if (k == 0) { i = si; j = sj; }
                else if (k == 1) { i = N - 1 - sj; j = si; }
                else if (k == 2) { i = N - 1 - si; j = N - 1 - sj; }
                else { i = sj; j = N - 1 - si; }
                const uint64_t p = (uint64_t)(i * N + j);
                uint64_t xk = sm64((p << 32) | b0);
                xk = sm64(xk ^ (((uint64_t)b1 << 32) | b2));
                lo += xk;
                hi += sm64(xk ^ 0xD6E8FEB86659FD93ull);
            }
        }
        lo = group_sum_u64<GL>(lo);
        hi = group_sum_u64<GL>(hi);
        if (valid && sl == 0) { key_out[2 * (size_t)pi] = lo; key_out[2 * (size_t)pi + 1] = hi; }
    }
    GAME_SYNC();                                           // the LDS region is reused by the next observation
    }
}

// ------------------------------------------------------------------------------------------
// deterministic stream compaction: indices of non-zero flags, ascending
// ------------------------------------------------------------------------------------------
#define CMP_THREADS 256
#define CMP_ITEMS 8
#define CMP_TILE (CMP_THREADS * CMP_ITEMS)

__device__ static inline int block_exclusive_scan_256(int v, int *total, int *sh /* >= 8 ints */)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(CMP_THREADS) void k_cmp_count(const uint8_t *__restrict__ flags, int n, int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * CMP_TILE + threadIdx.x * CMP_ITEMS;
    int c = 0;
    for (int q = 0; q < CMP_ITEMS; ++q) { const int i = base + q; if (i < n && flags[i]) ++c; }
    int total;
    block_exclusive_scan_256(c, &total, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// single block: exclusive scan of tile sums (any count, processed 256 at a time)
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_scan(int32_t *__restrict__ tile_sums, int n_tiles, int32_t *__restrict__ count)
{
    __shared__ int sh[8];
    int carry = 0;
    for (int b = 0; b < n_tiles; b += CMP_THREADS) {
        const int i = b + threadIdx.x;
        const int v = i < n_tiles ? tile_sums[i] : 0;
        int total;
        const int ex = block_exclusive_scan_256(v, &total, sh);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(CMP_THREADS) void k_cmp_scatter(const uint8_t *__restrict__ flags, int n, const int32_t *__restrict__ tile_offs,
                                                             int32_t *__restrict__ out)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * CMP_TILE + threadIdx.x * CMP_ITEMS;
    int c = 0;
    uint8_t f[CMP_ITEMS];
    for (int q = 0; q < CMP_ITEMS; ++q) { const int i = base + q; f[q] = (i < n) ? flags[i] : 0; if (f[q]) ++c; }
    int total;
    int pos = tile_offs[blockIdx.x] + block_exclusive_scan_256(c, &total, sh);
    for (int q = 0; q < CMP_ITEMS; ++q) if (f[q]) out[pos++] = base + q;
}

// the same compaction in ONE launch for lists a single block walks quickly (the rollout ticks of small and medium batches are
// bound by their launch count): every thread takes a run of consecutive flags; same output order as the three-kernel form
#define CMP_ONE_MAX (CMP_THREADS * 64)
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_one(const uint8_t *__restrict__ flags, int n, int32_t *__restrict__ out,
                                                         int32_t *__restrict__ count)
{
    __shared__ int sh[8];
    const int per = (n + CMP_THREADS - 1) / CMP_THREADS, base = threadIdx.x * per;
    int c = 0;
    for (int q = 0; q < per; ++q) { const int i = base + q; if (i < n && flags[i]) ++c; }
    int total;
    int pos = block_exclusive_scan_256(c, &total, sh);
    for (int q = 0; q < per; ++q) { const int i = base + q; if (i < n && flags[i]) out[pos++] = i; }
    if (threadIdx.x == 0) *count = total;
}

// ------------------------------------------------------------------------------------------
// the pit's row list and verdict (pit_mp_game_runner.py:23-35, 39-62) on the device: games are slots 0..n-1, `live` marks the
// games whose verdict is still open, snakes with id < a_cnt are team A
// ------------------------------------------------------------------------------------------
#define PIT_ITEMS 4
#define PIT_TILE (CMP_THREADS * PIT_ITEMS)      // games per block

// bit s = snake s of the record in `slot` is alive
__device__ static inline uint32_t slot_alive_bits(const uint8_t *__restrict__ state, const Layout &L, int slot)
{
    const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)slot * L.stride + L.meta_off);
    uint32_t bits = 0u;
    for (int s = 0; s < L.S; ++s) bits |= (meta[s].alive ? 1u : 0u) << s;
    return bits;
}

// the same of game gi; 0 for a game that is closed (or past the end)
__device__ static inline uint32_t pit_alive_bits(const uint8_t *__restrict__ state, const Layout &L, const uint8_t *live, int gi, int n)
{
    return gi < n && live[gi] ? slot_alive_bits(state, L, gi) : 0u;
}

// rows of each team in the block's PIT_TILE games: tile_sums[2 b] team A, [2 b + 1] team B
__global__ __launch_bounds__(CMP_THREADS) void k_pit_count(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                           int n, uint32_t a_bits, int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    int ca = 0, cb = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) {
        const uint32_t b = pit_alive_bits(state, L, live, base + q, n);
        ca += __popc(b & a_bits);
        cb += __popc(b & ~a_bits);
    }
    int ta, tb;
    block_exclusive_scan_256(ca, &ta, sh);
    block_exclusive_scan_256(cb, &tb, sh);
    if (threadIdx.x == 0) { tile_sums[2 * blockIdx.x] = ta; tile_sums[2 * blockIdx.x + 1] = tb; }
}

// single block: exclusive scan of both columns of the tile sums (any count, 256 tiles at a time); counts = {nA, nB}
__global__ __launch_bounds__(CMP_THREADS) void k_pit_scan(int32_t *__restrict__ tile_sums, int n_tiles, int32_t *__restrict__ counts)
{
    __shared__ int sh[8];
    int carry_a = 0, carry_b = 0;
    for (int b = 0; b < n_tiles; b += CMP_THREADS) {
        const int i = b + threadIdx.x;
        const int va = i < n_tiles ? tile_sums[2 * i] : 0, vb = i < n_tiles ? tile_sums[2 * i + 1] : 0;
        int ta, tb;
        const int ea = block_exclusive_scan_256(va, &ta, sh);
        const int eb = block_exclusive_scan_256(vb, &tb, sh);
        if (i < n_tiles) { tile_sums[2 * i] = carry_a + ea; tile_sums[2 * i + 1] = carry_b + eb; }
        carry_a += ta; carry_b += tb;
    }
    if (threadIdx.x == 0) { counts[0] = carry_a; counts[1] = carry_b; }
}

// team-A rows at [0, nA), team-B rows at [nA, nA + nB); inside a team games ascending, ids ascending (ids_A + ids_B)
__global__ __launch_bounds__(CMP_THREADS) void k_pit_scatter(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                             int n, uint32_t a_bits, const int32_t *__restrict__ tile_offs,
                                                             const int32_t *__restrict__ counts, int32_t *__restrict__ pairs)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    uint32_t bits[PIT_ITEMS];
    int ca = 0, cb = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) {
        bits[q] = pit_alive_bits(state, L, live, base + q, n);
        ca += __popc(bits[q] & a_bits);
        cb += __popc(bits[q] & ~a_bits);
    }
    int ta, tb;
    int pa = tile_offs[2 * blockIdx.x] + block_exclusive_scan_256(ca, &ta, sh);
    int pb = counts[0] + tile_offs[2 * blockIdx.x + 1] + block_exclusive_scan_256(cb, &tb, sh);
    for (int q = 0; q < PIT_ITEMS; ++q) {
        for (uint32_t b = bits[q]; b; b &= b - 1u) {          // a closed or absent game has no bit set
            const int s = __ffs((int)b) - 1;
            const int pos = ((a_bits >> s) & 1u) ? pa++ : pb++;
            pairs[2 * (size_t)pos] = base + q;
            pairs[2 * (size_t)pos + 1] = s;
        }
    }
}

// the root games of a searching side (agent.py:25-99 behind pit_mp_game_runner.py:23-38): the open slots ascending, what
// DeviceMCTS.search takes as live_slots / root_alive.  Open games of the block's PIT_TILE games: tile_sums[b]; the tile sums
// are scanned by k_cmp_scan (one column), which also writes the count G
__global__ __launch_bounds__(CMP_THREADS) void k_pit_roots_count(const uint8_t *__restrict__ live, int n, int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    int c = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) { const int gi = base + q; if (gi < n && live[gi]) ++c; }
    int total;
    block_exclusive_scan_256(c, &total, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// slots[j] = the j-th open slot, alive[j][s] = its snakes' alive flags, rank[slot] = j (-1 for a closed game); nothing past G
__global__ __launch_bounds__(CMP_THREADS) void k_pit_roots_scatter(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                                   int n, const int32_t *__restrict__ tile_offs, int32_t *__restrict__ slots,
                                                                   uint8_t *__restrict__ alive, int32_t *__restrict__ rank)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    bool open[PIT_ITEMS];
    int c = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) { const int gi = base + q; open[q] = gi < n && live[gi]; if (open[q]) ++c; }
    int total;
    int pos = tile_offs[blockIdx.x] + block_exclusive_scan_256(c, &total, sh);
    for (int q = 0; q < PIT_ITEMS; ++q) {
        const int gi = base + q;
        if (gi >= n) break;
        if (!open[q]) { rank[gi] = -1; continue; }
        const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)gi * L.stride + L.meta_off);
        for (int s = 0; s < L.S; ++s) alive[(size_t)pos * L.S + s] = meta[s].alive ? 1 : 0;
        slots[pos] = gi;
        rank[gi] = pos++;
    }
}

// the verdict of one turn (pit_mp_game_runner.py:39-62), a thread per game
__global__ void k_pit_verdict(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ done,
                              const int8_t *__restrict__ rewards, int n, uint32_t a_bits, int turn, uint8_t *live,
                              int32_t *__restrict__ winner, int32_t *__restrict__ length)
{
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n || !live[gi]) return;
    int w = -1;
    if (done[gi]) {                                           // :43-47 the last id whose reward is +1, None without one
        for (int s = 0; s < L.S; ++s) if (rewards[(size_t)gi * L.S + s] == 1) w = s;
    } else {                                                  // :48-60 a team without snakes: the first alive id wins
        const uint32_t b = pit_alive_bits(state, L, live, gi, n);
        if ((b & a_bits) && (b & ~a_bits)) return;            // both teams present: the game stays open
        w = b ? __ffs((int)b) - 1 : -1;
    }
    winner[gi] = w;
    length[gi] = turn;
    live[gi] = 0;
}

// ------------------------------------------------------------------------------------------
// the same row list and verdict with an owner per seat (snake_engine/league.py): owner[g][s] in 0..K-1 replaces the team split
// s < a_cnt, the rows are bucketed by owner, a game's verdict is in when at most one owner has snakes left
// ------------------------------------------------------------------------------------------
// byte s = the owner of seat s of game gi if that snake is alive, the game open and the owner below K; 0xFF otherwise
__device__ static inline uint64_t lg_owner_bytes(const uint8_t *__restrict__ state, const Layout &L, const uint8_t *live,
                                                 const uint8_t *__restrict__ owner, int K, int gi, int n)
{
    uint64_t w = ~0ull;
    if (gi >= n || !live[gi]) return w;
    const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)gi * L.stride + L.meta_off);
    for (int s = 0; s < L.S; ++s) {
        const uint32_t o = owner[(size_t)gi * L.S + s];
        if (meta[s].alive && o < (uint32_t)K) w = (w & ~(0xFFull << (8 * s))) | ((uint64_t)o << (8 * s));
    }
    return w;
}

// how many of the eight bytes of w equal o
__device__ static inline int lg_count_bytes(uint64_t w, uint32_t o)
{
    int c = 0;
#pragma unroll
    for (int s = 0; s < SNK_MAX_SNAKES; ++s) c += ((uint32_t)(w >> (8 * s)) & 0xFFu) == o ? 1 : 0;
    return c;
}

// rows of each owner in the block's PIT_TILE games: tile_sums[K b + o], a block scan per owner (column by column)
__global__ __launch_bounds__(CMP_THREADS) void k_lg_count(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                          int n, const uint8_t *__restrict__ owner, int K, int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    uint64_t w[PIT_ITEMS];
    for (int q = 0; q < PIT_ITEMS; ++q) w[q] = lg_owner_bytes(state, L, live, owner, K, base + q, n);
    for (int o = 0; o < K; ++o) {
        int c = 0;
        for (int q = 0; q < PIT_ITEMS; ++q) c += lg_count_bytes(w[q], (uint32_t)o);
        int total;
        block_exclusive_scan_256(c, &total, sh);
        if (threadIdx.x == 0) tile_sums[(size_t)K * blockIdx.x + o] = total;
    }
}

// single block: exclusive scan of every column of the tile sums (any count, 256 tiles at a time); counts[o] = owner o's rows
__global__ __launch_bounds__(CMP_THREADS) void k_lg_scan(int32_t *__restrict__ tile_sums, int n_tiles, int K, int32_t *__restrict__ counts)
{
    __shared__ int sh[8];
    for (int o = 0; o < K; ++o) {
        int carry = 0;
        for (int b = 0; b < n_tiles; b += CMP_THREADS) {
            const int i = b + threadIdx.x;
            const int v = i < n_tiles ? tile_sums[(size_t)K * i + o] : 0;
            int total;
            const int ex = block_exclusive_scan_256(v, &total, sh);
            if (i < n_tiles) tile_sums[(size_t)K * i + o] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) counts[o] = carry;
    }
}

// owner o's rows at [sum of counts below o, + counts[o]); inside an owner games ascending, ids ascending
__global__ __launch_bounds__(CMP_THREADS) void k_lg_scatter(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                            int n, const uint8_t *__restrict__ owner, int K,
                                                            const int32_t *__restrict__ tile_offs, const int32_t *__restrict__ counts,
                                                            int32_t *__restrict__ pairs)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    uint64_t w[PIT_ITEMS];
    for (int q = 0; q < PIT_ITEMS; ++q) w[q] = lg_owner_bytes(state, L, live, owner, K, base + q, n);
    int owner_base = 0;
    for (int o = 0; o < K; ++o) {
        int c = 0;
        for (int q = 0; q < PIT_ITEMS; ++q) c += lg_count_bytes(w[q], (uint32_t)o);
        int total;
        int pos = owner_base + tile_offs[(size_t)K * blockIdx.x + o] + block_exclusive_scan_256(c, &total, sh);
        if (c) {
            for (int q = 0; q < PIT_ITEMS; ++q) {
#pragma unroll
                for (int s = 0; s < SNK_MAX_SNAKES; ++s) {
                    if (((uint32_t)(w[q] >> (8 * s)) & 0xFFu) == (uint32_t)o) {
                        pairs[2 * (size_t)pos] = base + q;
                        pairs[2 * (size_t)pos + 1] = s;
                        ++pos;
                    }
                }
            }
        }
        owner_base += counts[o];
    }
}

// the verdict of one turn with an owner per seat (pit_mp_game_runner.py:39-62), a thread per game
__global__ void k_lg_verdict(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ done,
                             const int8_t *__restrict__ rewards, int n, const uint8_t *__restrict__ owner, int turn, uint8_t *live,
                             int32_t *__restrict__ winner, int32_t *__restrict__ winner_owner, int32_t *__restrict__ length)
{
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n || !live[gi]) return;
    const uint8_t *own = owner + (size_t)gi * L.S;
    int w = -1;
    if (done[gi]) {                                           // :43-47 the last id whose reward is +1, None without one
        for (int s = 0; s < L.S; ++s) if (rewards[(size_t)gi * L.S + s] == 1) w = s;
    } else {                                                  // :48-60 at most one owner left: the first alive id wins
        const uint32_t b = pit_alive_bits(state, L, live, gi, n);
        if (b) {
            w = __ffs((int)b) - 1;
            const uint8_t first = own[w];
            for (int s = w + 1; s < L.S; ++s)
                if (((b >> s) & 1u) && own[s] != first) return;   // two owners present: the game stays open
        }
    }
    winner[gi] = w;
    winner_owner[gi] = w >= 0 ? (int32_t)own[w] : -1;
    length[gi] = turn;
    live[gi] = 0;
}

// ------------------------------------------------------------------------------------------
// the root games of every searching owner (agent.py:25-99 behind pit_mp_game_runner.py:23-38 with an owner per seat): owner o's
// list is the open games in which a snake of o is alive, the lists stand one after another in owner order (k_pit_roots_* bucketed
// the way k_lg_* bucket the rows).  search_mask bit o = owner o searches; an owner outside the mask has no list
// ------------------------------------------------------------------------------------------
// games of each searching owner in the block's PIT_TILE games: tile_sums[K b + o] (0 for an owner outside the mask), which
// k_lg_scan scans column by column
__global__ __launch_bounds__(CMP_THREADS) void k_lgs_count(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                           int n, const uint8_t *__restrict__ owner, int K, uint32_t search_mask,
                                                           int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    uint64_t w[PIT_ITEMS];
    for (int q = 0; q < PIT_ITEMS; ++q) w[q] = lg_owner_bytes(state, L, live, owner, K, base + q, n);
    for (int o = 0; o < K; ++o) {
        int total = 0;
        if ((search_mask >> o) & 1u) {                        // the mask is the same for every thread of the block
            int c = 0;
            for (int q = 0; q < PIT_ITEMS; ++q) c += lg_count_bytes(w[q], (uint32_t)o) ? 1 : 0;
            block_exclusive_scan_256(c, &total, sh);
        }
        if (threadIdx.x == 0) tile_sums[(size_t)K * blockIdx.x + o] = total;
    }
}

// owner o's games at [sum of counts below o, + counts[o]), slots ascending: slots[r] = the game, alive[r][s] = the alive flags
// of ALL its snakes, rank[g][s] = r for an alive seat of o in that game; every other cell of rank takes -1.  Every cell of rank
// is written once, by the thread of its game; nothing past the sum of the counts is written
__global__ __launch_bounds__(CMP_THREADS) void k_lgs_scatter(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                             int n, const uint8_t *__restrict__ owner, int K, uint32_t search_mask,
                                                             const int32_t *__restrict__ tile_offs, const int32_t *__restrict__ counts,
                                                             int32_t *__restrict__ slots, uint8_t *__restrict__ alive,
                                                             int32_t *__restrict__ rank)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    uint64_t w[PIT_ITEMS];
    for (int q = 0; q < PIT_ITEMS; ++q) {
        const int gi = base + q;
        w[q] = lg_owner_bytes(state, L, live, owner, K, gi, n);
        if (gi >= n) continue;
        for (int s = 0; s < L.S; ++s) {                       // a seat no list covers: dead, closed, no owner, or a greedy owner
            const uint32_t o = (uint32_t)(w[q] >> (8 * s)) & 0xFFu;
            if (o == 0xFFu || !((search_mask >> o) & 1u)) rank[(size_t)gi * L.S + s] = -1;
        }
    }
    int owner_base = 0;
    for (int o = 0; o < K; ++o) {
        if (!((search_mask >> o) & 1u)) continue;             // counts[o] is 0
        int c = 0;
        for (int q = 0; q < PIT_ITEMS; ++q) c += lg_count_bytes(w[q], (uint32_t)o) ? 1 : 0;
        int total;
        int pos = owner_base + tile_offs[(size_t)K * blockIdx.x + o] + block_exclusive_scan_256(c, &total, sh);
        if (c) {
            for (int q = 0; q < PIT_ITEMS; ++q) {
                if (!lg_count_bytes(w[q], (uint32_t)o)) continue;     // never true for a game past the end: its bytes are 0xFF
                const int gi = base + q;
                const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)gi * L.stride + L.meta_off);
                for (int s = 0; s < L.S; ++s) {
                    alive[(size_t)pos * L.S + s] = meta[s].alive ? 1 : 0;
                    if (((uint32_t)(w[q] >> (8 * s)) & 0xFFu) == (uint32_t)o) rank[(size_t)gi * L.S + s] = pos;
                }
                slots[pos++] = gi;
            }
        }
        owner_base += counts[o];
    }
}

// ------------------------------------------------------------------------------------------
// the scripted opponent of the pit (snake_engine.arena.Scripted): the three move scores of every row of a row list, from the
// compact records alone -- no observation, no net.  The policy is the project's own (the reference has no scripted snake); it is
// stated in include/snake_engine.h and, in plain Python, in tests/script_ref.py.
// A quad of lanes per row, sixteen rows per wavefront.  All four lanes build the occupancy bit plane of the row's game (lane k
// walks the rings of snakes k and k + 4) and OR it across the quad with two DPP quad_perm moves per half word; lanes 0..2 then
// each score one move, the flood fill as whole-plane shifts of a reach mask.  The plane is FW 64-bit words in registers (FW = 1:
// up to 64 cells, 2: up to 128, 6: up to 361), every loop over them unrolled, so no array is indexed by a run-time value.
// Every loop is bounded whatever the record holds: a ring walk by min(len, cap), the fill by NC rounds, the food scan by the
// bits of a word; a cell index is compared with NC before it sets a bit.  The DPP moves are the only cross-lane operations and
// no lane has left when they run: a row without a snake (a dead or out-of-range pair, a row past m) walks nothing, takes part
// with an empty plane and writes its three -1 (past m: nothing) at the end.
// ------------------------------------------------------------------------------------------
struct ScriptMasks {
    uint64_t valid[6];      // bit c = c < NC
    uint64_t not_c0[6];     // bit c = c < NC and c % W != 0: a cell that has a left neighbour
    uint64_t not_cl[6];     // bit c = c < NC and c % W != W - 1: a cell that has a right neighbour
};

static ScriptMasks script_masks(const Layout &L)
{
    ScriptMasks K;
    memset(&K, 0, sizeof(K));
    for (int c = 0; c < L.NC; ++c) {
        const uint64_t bit = 1ull << (c & 63);
        K.valid[c >> 6] |= bit;
        if (c % L.W != 0) K.not_c0[c >> 6] |= bit;
        if (c % L.W != L.W - 1) K.not_cl[c >> 6] |= bit;
    }
    return K;
}

__device__ static inline int script_ring_cell(const uint8_t *rec, const Layout &L, int s, int idx)
{
    const uint8_t *r = rec + (size_t)s * L.ring_bytes;
    idx &= L.cap_mask;
    return L.cell_bytes == 1 ? (int)r[idx] : (int)((const uint16_t *)r)[idx];
}

// ---- what the two one-launch scorers share (k_pit_script here, k_pit_territory below): each kernel states only its own part
// a lane's row: lane k of the quad of row `row`, the row's pair (slot, snake s) decoded and guarded.  in: the row is below m; ok:
// the pair names an alive snake of a slot of the engine -- when it does not, rec is slot 0's record and nothing of it is read
struct ScriptRow {
    int row, k, s;
    bool in, ok;
    const uint8_t *rec;
    const SnakeMeta *meta;
    SnakeMeta me;
};

__device__ __forceinline__ ScriptRow script_row(const uint8_t *__restrict__ state, const Layout &L, int n_slots,
                                                const int32_t *__restrict__ pairs, int m)
{
    const int t = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    ScriptRow R;
    R.row = t >> 2;
    R.k = t & 3;
    R.in = R.row < m;
    int g = -1;
    R.s = -1;
    if (R.in) { g = pairs[2 * (size_t)R.row]; R.s = pairs[2 * (size_t)R.row + 1]; }
    const bool pair_ok = R.in && g >= 0 && g < n_slots && R.s >= 0 && R.s < L.S;
    R.rec = state + (size_t)(pair_ok ? g : 0) * L.stride;
    R.meta = (const SnakeMeta *)(R.rec + L.meta_off);
    R.me = {0, 0, 0, 0, 0};
    if (pair_ok) R.me = R.meta[R.s];
    R.ok = pair_ok && R.me.alive;
    return R;
}

// the ring cells of snake o (its meta mo) into a plane: tails and all, min(len, cap) steps
template <int FW>
__device__ __forceinline__ void script_mark_ring(const ScriptRow &R, const Layout &L, int o, const SnakeMeta &mo, uint64_t (&occ)[FW])
{
    const int len = (int)mo.len < L.cap ? (int)mo.len : L.cap;
    for (int i = 0; i < len; ++i) {
        const int c = script_ring_cell(R.rec, L, o, mo.tail + i);
        if (c < L.NC) {
#pragma unroll
            for (int w = 0; w < FW; ++w) occ[w] |= (c >> 6) == w ? 1ull << (c & 63) : 0ull;
        }
    }
}

// a plane ORed across the quad, every lane of it getting the whole.  Cross-lane: all 64 lanes of the wavefront must reach the call
template <int FW>
__device__ __forceinline__ void quad_or(uint64_t (&plane)[FW])
{
#pragma unroll
    for (int w = 0; w < FW; ++w) {
        int lo = (int)(uint32_t)plane[w], hi = (int)(uint32_t)(plane[w] >> 32);
        lo |= __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true);      // quad_perm [1,0,3,2]
        hi |= __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
        lo |= __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
        hi |= __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true);
        plane[w] = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
    }
}

// where relative move R.k takes the row's head: (y, x), its cell tc (0 off the board), and blocked = off the board or occupied
struct ScriptTarget {
    int y, x, tc;
    bool blocked;
};

template <int FW>
__device__ __forceinline__ ScriptTarget script_target(const ScriptRow &R, const Layout &L, const uint64_t (&occ)[FW])
{
    const int hc = script_ring_cell(R.rec, L, R.s, R.me.tail + (int)R.me.len - 1);
    const int d = (R.k + R.me.dir + 3) & 3;                   // k_step's heading: 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1
    ScriptTarget T;
    T.y = hc / L.W;
    T.x = hc - T.y * L.W;
    T.y += (d == 2) - (d == 0);
    T.x += (d == 1) - (d == 3);
    const bool oob = (T.y < 0) | (T.y >= L.H) | (T.x < 0) | (T.x >= L.W);
    T.tc = oob ? 0 : T.y * L.W + T.x;
    T.blocked = oob;
#pragma unroll
    for (int w = 0; w < FW; ++w) T.blocked |= (T.tc >> 6) == w && ((occ[w] >> (T.tc & 63)) & 1ull);
    return T;
}

// one round of growth: nx = r and its four neighbours inside fr, as whole-plane shifts
template <int FW>
__device__ __forceinline__ void script_grow(const uint64_t (&r)[FW], const uint64_t (&fr)[FW], const ScriptMasks &K, int WW,
                                            uint64_t (&nx)[FW])
{
#pragma unroll
    for (int w = 0; w < FW; ++w) {
        const uint64_t below = w > 0 ? r[w > 0 ? w - 1 : 0] : 0ull, above = w < FW - 1 ? r[w < FW - 1 ? w + 1 : 0] : 0ull;
        const uint64_t from_up = (r[w] << WW) | (below >> (64 - WW));         // cell c takes cell c - W
        const uint64_t from_dn = (r[w] >> WW) | (above << (64 - WW));         // cell c takes cell c + W
        const uint64_t from_lf = ((r[w] << 1) | (below >> 63)) & K.not_c0[w]; // cell c takes cell c - 1, not across a row end
        const uint64_t from_rt = ((r[w] >> 1) | (above << 63)) & K.not_cl[w]; // cell c takes cell c + 1
        nx[w] = (r[w] | from_up | from_dn | from_lf | from_rt) & fr[w];
    }
}

// the score of a move that is not blocked, from its space (the script) or territory.  safe: 0 when another alive snake at least as
// long as the row's has its head next to the target; food: H + W - the smallest Manhattan distance from the target to a food cell,
// 0 without food and for a row that is not `hungry` (the script's rows always are)
template <int FW>
__device__ __forceinline__ int script_score(const ScriptRow &R, const Layout &L, const ScriptMasks &K, uint32_t flags, bool hungry,
                                            const ScriptTarget &T, int space)
{
    const int len_s = R.me.len;
    int safe = 1;
    if (flags & SNK_SCRIPT_HEADS) {
        for (int o = 0; o < L.S; ++o) {
            if (o == R.s) continue;
            const SnakeMeta mo = R.meta[o];
            if (!mo.alive || (int)mo.len < len_s) continue;
            const int ho = script_ring_cell(R.rec, L, o, mo.tail + mo.len - 1);
            const int oy = ho / L.W, ox = ho - oy * L.W;
            if (abs(oy - T.y) + abs(ox - T.x) == 1) safe = 0;
        }
    }
    int food = 0;
    if ((flags & SNK_SCRIPT_FOOD) && hungry) {
        const uint64_t *fw = (const uint64_t *)(R.rec + L.food_off);
        int best = 1 << 20;
#pragma unroll
        for (int w = 0; w < FW; ++w) {
            uint64_t f = fw[w < L.FW ? w : 0] & K.valid[w];          // valid[] is 0 from the layout's word count up
            while (f) {                                              // one set bit less per pass: at most 64
                const int c = w * 64 + __builtin_ctzll(f);
                f &= f - 1ull;
                const int fy = c / L.W, fx = c - fy * L.W;
                const int dist = abs(fy - T.y) + abs(fx - T.x);
                best = dist < best ? dist : best;
            }
        }
        if (best != (1 << 20)) food = L.H + L.W - best;
    }
    int room = space < len_s ? space : len_s;
    room = room < 255 ? room : 255;
    const int fill = space < 511 ? space : 511;
    return ((room * 2 + safe) * 64 + food) * 512 + fill;
}

template <int FW>
__global__ __launch_bounds__(BLOCK_THREADS) void k_pit_script(const uint8_t *__restrict__ state, Layout L, int n_slots,
                                                             const int32_t *__restrict__ pairs, int m, uint32_t flags,
                                                             ScriptMasks K, float *__restrict__ q)
{
    const ScriptRow R = script_row(state, L, n_slots, pairs, m);

    // ---- occupied: every ring cell of every alive snake, tails and the row's own body included
    uint64_t occ[FW];
#pragma unroll
    for (int w = 0; w < FW; ++w) occ[w] = 0ull;
    if (R.ok) {
        for (int o = R.k; o < L.S; o += 4) {
            const SnakeMeta mo = R.meta[o];
            if (mo.alive) script_mark_ring<FW>(R, L, o, mo, occ);
        }
    }
    quad_or<FW>(occ);                                 // all 64 lanes are here: the quad's four partial planes become one

    // ---- lane k < 3 scores relative move k
    int score = -1;
    if (R.ok && R.k < 3) {
        const ScriptTarget T = script_target<FW>(R, L, occ);
        if (!T.blocked) {
            int space = 0;
            if (flags & SNK_SCRIPT_SPACE) {           // the flood fill: a reach mask grown from the target until it stops
                uint64_t fr[FW], r[FW], nx[FW];
#pragma unroll
                for (int w = 0; w < FW; ++w) {
                    fr[w] = ~occ[w] & K.valid[w];
                    r[w] = (T.tc >> 6) == w ? 1ull << (T.tc & 63) : 0ull;
                }
                for (int round = 0; round < L.NC; ++round) {  // a round that changes the mask adds a cell: at most NC - 1 of them
                    script_grow<FW>(r, fr, K, L.W, nx);
                    bool changed = false;
#pragma unroll
                    for (int w = 0; w < FW; ++w) {
                        changed |= nx[w] != r[w];
                        r[w] = nx[w];
                    }
                    if (!changed) break;
                }
#pragma unroll
                for (int w = 0; w < FW; ++w) space += __popcll(r[w]);
            }
            score = script_score<FW>(R, L, K, flags, true, T, space);
        }
    }
    if (R.in && R.k < 3) q[3 * (size_t)R.row + R.k] = (float)score;
}

// ------------------------------------------------------------------------------------------
// the territory opponent of the pit (snake_engine.arena.Territory, snk_pit_territory_values): the scripted policy with Voronoi
// territory -- the free cells the snake reaches before anybody else does -- in place of the flood fill's space.  The policy is the
// project's own; include/snake_engine.h states it and tests/territory_ref.py restates it in plain Python.
// k_pit_script's form: a quad of lanes per row, planes as FW words in registers, every loop unrolled or bounded whatever the record
// holds.  While lane k walks the rings of snakes k and k + 4 for the occupancy plane it also sets, for each of them that is not the
// row's own snake, the on-board targets of its three moves in one of two start planes: `strong` for a snake at least as long as
// the row's, `weak` for a shorter one.  The three planes are ORed across the quad by the same DPP moves, so the start planes are
// built once per row; no lane has left when they run (flags is the same in every lane).  Lanes 0..2 then each score one move.
// The fronts expand freely over the free cells, a round per step of distance, by the four shifts of script_grow.  A cell that
// my front reaches first in round r is mine when no strong front has reached it by round r and no weak front before round r
// (the head-on rule).  "Before round r" is "by round r" of a front that starts one round late, and growing distributes over OR,
// so the strong and the late weak fronts are ONE plane `their`: the strong starts, grown once, joined by the weak starts -- that
// is round 1 -- and grown once a round from there on.  Two fronts are carried, and the weak start plane is dead before the loop.
// The rounds end when my front stops growing, and after NC of them at the latest.
// ------------------------------------------------------------------------------------------
template <int FW>
__global__ __launch_bounds__(BLOCK_THREADS) void k_pit_territory(const uint8_t *__restrict__ state, Layout L, int n_slots,
                                                                const int32_t *__restrict__ pairs, int m, uint32_t flags,
                                                                int hungry, ScriptMasks K, float *__restrict__ q)
{
    const ScriptRow R = script_row(state, L, n_slots, pairs, m);
    const bool fronts = (flags & SNK_SCRIPT_SPACE) != 0u;     // the same in every lane
    const int HH = L.H, WW = L.W;
    const int len_s = R.me.len;

    // ---- occupied as in k_pit_script; strong and weak: where the other alive snakes can stand after this tick (free or not)
    uint64_t occ[FW], strong[FW], weak[FW];
#pragma unroll
    for (int w = 0; w < FW; ++w) occ[w] = strong[w] = weak[w] = 0ull;
    if (R.ok) {
        for (int o = R.k; o < L.S; o += 4) {
            const SnakeMeta mo = R.meta[o];
            if (!mo.alive) continue;
            script_mark_ring<FW>(R, L, o, mo, occ);
            if (!fronts || o == R.s) continue;
            const int ho = script_ring_cell(R.rec, L, o, mo.tail + mo.len - 1);
            const int oy = ho / WW, ox = ho - oy * WW;
            const bool is_strong = (int)mo.len >= len_s;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int d = (a + mo.dir + 3) & 3;
                const int y = oy + (d == 2) - (d == 0), x = ox + (d == 1) - (d == 3);
                if ((y < 0) | (y >= HH) | (x < 0) | (x >= WW)) continue;
                const int c = y * WW + x;                     // on the board: below NC
#pragma unroll
                for (int w = 0; w < FW; ++w) {
                    const uint64_t bit = (c >> 6) == w ? 1ull << (c & 63) : 0ull;
                    strong[w] |= is_strong ? bit : 0ull;
                    weak[w] |= is_strong ? 0ull : bit;
                }
            }
        }
    }
    quad_or<FW>(occ);                                 // all 64 lanes are here: the quad's four partial planes become one
    if (fronts) {
        quad_or<FW>(strong);
        quad_or<FW>(weak);
    }

    // ---- lane k < 3 scores relative move k
    int score = -1;
    if (R.ok && R.k < 3) {
        const ScriptTarget T = script_target<FW>(R, L, occ);
        if (!T.blocked) {
            int territory = 0;
            if (fronts) {
                uint64_t fr[FW], mine[FW], their[FW], nx[FW];
#pragma unroll
                for (int w = 0; w < FW; ++w) {
                    fr[w] = ~occ[w] & K.valid[w];
                    mine[w] = (T.tc >> 6) == w ? 1ull << (T.tc & 63) : 0ull;      // the target is free
                    strong[w] &= fr[w];
                    territory += __popcll(mine[w] & ~strong[w]);                  // round 0: no weak front yet
                }
                script_grow<FW>(strong, fr, K, WW, their);                        // round 1: the strong fronts at distance <= 1
#pragma unroll
                for (int w = 0; w < FW; ++w) their[w] |= weak[w] & fr[w];         //          and the weak ones at distance 0
                for (int round = 1; round < L.NC; ++round) {  // a round that changes my front adds a cell: at most NC - 1 of them
                    script_grow<FW>(mine, fr, K, WW, nx);
                    bool changed = false;
#pragma unroll
                    for (int w = 0; w < FW; ++w) {
                        const uint64_t fresh = nx[w] & ~mine[w];
                        changed |= fresh != 0ull;
                        territory += __popcll(fresh & ~their[w]);
                        mine[w] = nx[w];
                    }
                    if (!changed) break;
                    script_grow<FW>(their, fr, K, WW, nx);
#pragma unroll
                    for (int w = 0; w < FW; ++w) their[w] = nx[w];
                }
            }
            score = script_score<FW>(R, L, K, flags, (int)R.me.health <= hungry, T, territory);
        }
    }
    if (R.in && R.k < 3) q[3 * (size_t)R.row + R.k] = (float)score;
}

// ------------------------------------------------------------------------------------------
// the lookahead opponent of the pit (snake_engine.arena.Lookahead, snk_pit_look_values): the scripted policy one tick deep.  The
// policy is the project's own; include/snake_engine.h states it and tests/look_ref.py restates it in plain Python.  A row (slot g,
// snake s) of a game with A = 2..4 snakes alive is scored over the 3^A children of its game: copies made by k_clone, stepped once
// by the step kernels on a sub-engine without food spawning, and scored by k_pit_script -- launched by the entry point through
// snk_engine_clone, snk_engine_step_active and snk_pit_script_values.  It is the deep opponent below at depth 1: the entry point,
// the scratch (DeepScratch) and the fold (k_deep_reduce, level 0 as the parent) are that one's.  What is the lookahead's own:
//   k_look_count / k_cmp_scan / k_look_groups   the plan's scan over the rows (the three launches of k_pit_roots_*: tile sums, one
//                                               block scanning them, the scatter): rows of one slot that stand next to each other
//                                               form a group and share one set of children; per group its source slot and the
//                                               alive bits of that slot
//   k_look_fan                                  the plan's fan-out, a thread per child and per leaf: the children's active flags and
//                                               dense moves, and the leaf pair list (sub slot, s) the script kernel scores --
//                                               k_deep_fan and k_deep_leaves of a one-level tree in one launch
// Every cell of every array has one writer, nothing is read back, and there are no atomics.  All per-thread state is scalar: no
// array is indexed by a run-time value.
// ------------------------------------------------------------------------------------------
#define LK_MAX_LEAVES (1 << 28)                  // m * F: a quad of lanes per leaf row of the script kernel stays inside an int
#define LK_WIN 16777216.0f                       // 2^24: above every plain score

__host__ __device__ static inline int look_pow3(int k) { int p = 1; for (int i = 0; i < k; ++i) p *= 3; return p; }

// row i starts a group when it is row 0 or names another slot than row i - 1
__device__ static inline bool look_starts(const int32_t *__restrict__ pairs, int i)
{
    return i == 0 || pairs[2 * (size_t)i] != pairs[2 * (size_t)i - 2];
}

// groups that start in the block's PIT_TILE rows: tile_sums[b]
__global__ __launch_bounds__(CMP_THREADS) void k_look_count(const int32_t *__restrict__ pairs, int m, int32_t *__restrict__ tile_sums)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    int c = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) { const int i = base + q; if (i < m && look_starts(pairs, i)) ++c; }
    int total;
    block_exclusive_scan_256(c, &total, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// row_group[i] = the group of row i (any size: the reduce compares it with n_groups); for a group g < n_groups the row that starts
// it writes its source slot and alive bits -- slot 0 and no bits for a slot outside the engine --, and the groups from the count
// up to n_groups, which no row starts, get slot 0 and no bits from the thread whose rows have their numbers (n_groups <= m)
__global__ __launch_bounds__(CMP_THREADS) void k_look_groups(const uint8_t *__restrict__ state, Layout L, int n_slots,
                                                            const int32_t *__restrict__ pairs, int m, const int32_t *__restrict__ tile_offs,
                                                            const int32_t *__restrict__ count, int n_groups,
                                                            int32_t *__restrict__ row_group, int32_t *__restrict__ grp_src,
                                                            int32_t *__restrict__ grp_bits)
{
    __shared__ int sh[8];
    const int base = blockIdx.x * PIT_TILE + threadIdx.x * PIT_ITEMS;
    int c = 0;
    for (int q = 0; q < PIT_ITEMS; ++q) { const int i = base + q; if (i < m && look_starts(pairs, i)) ++c; }
    int total;
    int run = tile_offs[blockIdx.x] + block_exclusive_scan_256(c, &total, sh);        // groups started before this thread's rows
    const int groups = *count;
    for (int q = 0; q < PIT_ITEMS; ++q) {
        const int i = base + q;
        if (i >= m) break;
        const bool starts = look_starts(pairs, i);
        if (starts) ++run;
        const int g = run - 1;
        row_group[i] = g;
        if (starts && g < n_groups) {
            const int slot = pairs[2 * (size_t)i];
            const bool valid = slot >= 0 && slot < n_slots;
            uint32_t bits = 0u;
            if (valid) {
                const SnakeMeta *meta = (const SnakeMeta *)(state + (size_t)slot * L.stride + L.meta_off);
                for (int s = 0; s < L.S; ++s) bits |= (meta[s].alive ? 1u : 0u) << s;
            }
            grp_src[g] = valid ? slot : 0;
            grp_bits[g] = (int32_t)bits;
        }
        if (i >= groups && i < n_groups) { grp_src[i] = 0; grp_bits[i] = 0; }
    }
}

// thread t < n_groups * F is child j = t % F of group t / F: active when the group's game has A = 2..4 snakes alive and
// j < 3^A; its k-th alive snake moves (j / 3^k) % 3, every other entry is 1.  Thread t < m * F is leaf j of row t / F: the pair
// (sub slot of child j of the row's group, s) when the row is looked ahead and the child is active, else (-1, -1), which the
// script kernel scores -1, -1, -1 without walking anything
__global__ __launch_bounds__(CMP_THREADS) void k_look_fan(int m, int F, int S, int n_groups, const int32_t *__restrict__ pairs,
                                                         const int32_t *__restrict__ row_group, const int32_t *__restrict__ grp_bits,
                                                         uint8_t *__restrict__ active, uint8_t *__restrict__ moves,
                                                         int32_t *__restrict__ leaf_pairs)
{
    const int t = blockIdx.x * CMP_THREADS + threadIdx.x;
    const int g = t / F, j = t - g * F;                   // as a child: group and index; as a leaf: row and index
    if (g < n_groups) {
        const uint32_t bits = (uint32_t)grp_bits[g];
        const int A = __popc(bits);
        const bool act = A >= 2 && A <= 4 && j < look_pow3(A);
        active[t] = act ? 1 : 0;
        int d = j;
        for (int s = 0; s < S; ++s) {
            int mv = 1;
            if (act && ((bits >> s) & 1u)) { mv = d % 3; d /= 3; }
            moves[(size_t)t * S + s] = (uint8_t)mv;
        }
    }
    if (g < m) {
        const int s = pairs[2 * (size_t)g + 1], grp = row_group[g];
        bool look = false;
        if (grp < n_groups && s >= 0 && s < S) {
            const uint32_t bits = (uint32_t)grp_bits[grp];
            const int A = __popc(bits);
            look = ((bits >> s) & 1u) && A >= 2 && A <= 4 && j < look_pow3(A);
        }
        leaf_pairs[2 * (size_t)t] = look ? grp * F + j : -1;
        leaf_pairs[2 * (size_t)t + 1] = look ? s : -1;
    }
}

// ------------------------------------------------------------------------------------------
// the deep opponent of the pit (snake_engine.arena.Deep, snk_pit_deep_values): the scripted policy `depth` ticks deep, a paranoid
// fixed-depth search over the lookahead's children.  include/snake_engine.h states the policy, tests/deep_ref.py restates it in
// plain Python.  Depth 1 IS snk_pit_look_values (that entry point runs this body with one level).  The rows are grouped by the
// lookahead's scan (k_look_count / k_cmp_scan / k_look_groups), and the tree of a group stands in one sub-engine per level:
// node c of level k (slot c of subs[k-1]) is child c % F of node c / F of level k - 1; level 0 is the group's game.  What is new:
//   k_deep_fan      a thread per node of a level, after the level above has been stepped: the node is active when its parent is
//                   and has 2..4 snakes alive and the node's index is below 3^alive; its dense moves are the digits of that index
//   k_deep_leaves   a thread per (row, node of the last level): the pair (slot, s) the script kernel scores, (-1, -1) where the
//                   node is not active -- the only list that is per row; clones, flags and moves are per node, shared by the rows
//   k_deep_reduce   a quad of lanes per (row, node of the level above), lane a scores own move a over the node's children in
//                   which s's digit is a; the largest of the three goes to the level above, the three of level 0 are the result
// k_clone, the step kernels and k_pit_script do the rest, launched through their entry points.  Every cell of every array has one
// writer, nothing is read back, there are no atomics, and all per-thread state is scalar.  A node that is not active holds a
// stale record; no kernel reads it: the reduce visits the children of an active node with 2..4 alive only, and only the first
// 3^alive of them, which are the active ones.  Every node index is compared with its sub-engine's n_slots before it is used.
// ------------------------------------------------------------------------------------------
#define DP_MAX_DEPTH 4
#define DP_MAX_FANOUT 6561                       // F^depth: 3^8

// scratch, in int32 elements from its start; every part starts at a multiple of four elements (16 bytes)
struct DeepScratch {
    long tile_sums;                 // int32[tiles] + the group count
    long row_group;                 // int32[m]             the group of every row
    long grp_src;                   // int32[m]             a group's source slot (a valid slot for every group < n_groups)
    long grp_bits;                  // int32[m]             bit s = snake s of the source slot is alive; 0: the group is not searched
    long fb_q;                     // float[m][3]          the plain scores of the rows themselves
    long active[DP_MAX_DEPTH];      // uint8[m * F^k]       level k's flags for the step
    long moves[DP_MAX_DEPTH];       // uint8[m * F^k][S]
    long best[DP_MAX_DEPTH];        // float[m * F^k]       per (row, node of level k < depth): the best of s's three scores there
    long leaf_pairs;                // int32[m * F^depth][2]
    long leaf_q;                    // float[m * F^depth][3]
    long total;
};

static DeepScratch deep_scratch(long m, int S, int F, int depth)
{
    auto up4 = [](long v) { return (v + 3) / 4 * 4; };
    DeepScratch P;
    memset(&P, 0, sizeof(P));
    long at = 0, n = m;
    P.tile_sums = at;  at += up4((m + PIT_TILE - 1) / PIT_TILE + 1);
    P.row_group = at;  at += up4(m);
    P.grp_src = at;    at += up4(m);
    P.grp_bits = at;   at += up4(m);
    P.fb_q = at;       at += up4(3 * m);
    for (int k = 0; k < depth; ++k) {
        n *= F;
        P.active[k] = at;  at += up4((n + 3) / 4);
        P.moves[k] = at;   at += up4((n * S + 3) / 4);
        if (k + 1 < depth) { P.best[k] = at;  at += up4(n); }
    }
    P.leaf_pairs = at; at += up4(2 * n);
    P.leaf_q = at;     at += up4(3 * n);
    P.total = at;
    return P;
}

// thread t < n_nodes is node t of a level: child j = t % F of parent p = t / F.  par_state == nullptr: level 1, the parent is
// group p and grp_bits[p] its alive bits (0 for a group that is not looked ahead).  Otherwise the parent is slot p of the
// sub-engine above, after its step: a parent that was not active, or in which the game is over, has no children
__global__ __launch_bounds__(CMP_THREADS) void k_deep_fan(int n_nodes, int F, const int32_t *__restrict__ grp_bits,
                                                         const uint8_t *__restrict__ par_state, Layout L, int par_slots,
                                                         const uint8_t *__restrict__ par_active, uint8_t *__restrict__ active,
                                                         uint8_t *__restrict__ moves)
{
    const int t = blockIdx.x * CMP_THREADS + threadIdx.x;
    if (t >= n_nodes) return;
    const int p = t / F, j = t - p * F;
    uint32_t bits = 0u;
    if (par_state == nullptr) bits = (uint32_t)grp_bits[p];
    else if (p < par_slots && par_active[p]) bits = slot_alive_bits(par_state, L, p);
    const int A = __popc(bits);
    const bool act = A >= 2 && A <= 4 && j < look_pow3(A);
    active[t] = act ? 1 : 0;
    int d = j;
    for (int s = 0; s < L.S; ++s) {
        int mv = 1;
        if (act && ((bits >> s) & 1u)) { mv = d % 3; d /= 3; }
        moves[(size_t)t * L.S + s] = (uint8_t)mv;
    }
}

// thread t < m * FD is node l = t % FD of the last level of the tree of row t / FD: the pair (its slot, s) when the row is
// searched and the node active, else (-1, -1), which the script kernel scores -1, -1, -1 without walking anything
__global__ __launch_bounds__(CMP_THREADS) void k_deep_leaves(int m, int FD, int S, int n_groups, int leaf_slots,
                                                            const int32_t *__restrict__ pairs, const int32_t *__restrict__ row_group,
                                                            const int32_t *__restrict__ grp_bits, const uint8_t *__restrict__ active,
                                                            int32_t *__restrict__ leaf_pairs)
{
    const int t = blockIdx.x * CMP_THREADS + threadIdx.x;
    const int row = t / FD, l = t - row * FD;
    if (row >= m) return;
    const int s = pairs[2 * (size_t)row + 1], grp = row_group[row];
    bool ok = false;
    int node = -1;
    if (grp < n_groups && s >= 0 && s < S && (((uint32_t)grp_bits[grp] >> s) & 1u)) {
        node = grp * FD + l;                              // n_groups * FD <= leaf_slots <= 2^28
        ok = node < leaf_slots && active[node];
    }
    leaf_pairs[2 * (size_t)t] = ok ? node : -1;
    leaf_pairs[2 * (size_t)t + 1] = ok ? s : -1;
}

// the fold of level k into level k - 1.  A quad of lanes per (row, parent), P = F^(k-1) parents per row; lane a < 3 scores own
// move a at the parent over the 3^(A-1) children in which s's digit is a: the smallest child value when s lives in all of them,
// else -2 - (the children in which s is dead) - penalty, penalty = 32 * (the ticks below this level).  A child's value is 2^24
// when s alone is left in it, else what the level below stored for (row, child) -- at the last level (leaf_q != nullptr) the
// largest of s's three plain scores.  A parent is folded when it is active, s is alive in it and 2..4 snakes are.
//   P > 1 (par_state != nullptr): the largest of the three scores goes to best_out[row * P + parent], 0 for a parent not folded
//         (nothing reads that cell); the quad's lanes exchange their scores by two shuffles, which every lane of the wave runs
//   P == 1: the parent is the row's game.  q[row][a] = the score; the row's plain score fb_q when the row is not searched (a dead
//         or out-of-range pair, A < 2, A > 4); -1 when the row's group lies beyond the sub-engines
__global__ __launch_bounds__(CMP_THREADS) void k_deep_reduce(const uint8_t *__restrict__ par_state, int par_slots,
                                                            const uint8_t *__restrict__ par_active,
                                                            const uint8_t *__restrict__ cur_state, int cur_slots, Layout L, int m, int F,
                                                            int P, int n_groups, float penalty, const int32_t *__restrict__ pairs,
                                                            const int32_t *__restrict__ row_group, const int32_t *__restrict__ grp_bits,
                                                            const float *__restrict__ best_in, const float *__restrict__ leaf_q,
                                                            const float *__restrict__ fb_q, float *__restrict__ best_out,
                                                            float *__restrict__ q)
{
    const int t = blockIdx.x * CMP_THREADS + threadIdx.x;
    const int quad = t >> 2, a = t & 3;
    const int row = quad / P, pi = quad - row * P;
    const bool in = row < m;
    float val = -3.0e38f;
    bool fold = false, served = false;
    if (in) {
        const int s = pairs[2 * (size_t)row + 1], grp = row_group[row];
        served = grp < n_groups;
        uint32_t bits = 0u;
        int par = grp;                                    // the parent's node index: n_groups * P <= par_slots <= 2^28
        if (served) {
            if (par_state == nullptr) bits = (uint32_t)grp_bits[grp];
            else {
                par = grp * P + pi;
                if (par < par_slots && par_active[par]) bits = slot_alive_bits(par_state, L, par);
            }
        }
        const int A = __popc(bits);
        fold = s >= 0 && s < L.S && ((bits >> s) & 1u) && A >= 2 && A <= 4;
        if (fold && a < 3) {
            const int p = look_pow3(__popc(bits & ((1u << s) - 1u)));        // the weight of s's digit
            const int replies = look_pow3(A - 1);
            const uint32_t others = bits & ~(1u << s);
            const size_t mine = ((size_t)row * P + pi) * F;                  // the row's own index of the parent's child 0
            int dead = 0;
            float worst = LK_WIN;
            for (int i = 0; i < replies; ++i) {
                const int hi = i / p, j = hi * 3 * p + a * p + (i - hi * p);
                const long long node = (long long)par * F + j;
                if (node >= cur_slots) { ++dead; continue; }                 // never: the entry point sized the sub-engines
                const SnakeMeta *meta = (const SnakeMeta *)(cur_state + (size_t)node * L.stride + L.meta_off);
                if (!meta[s].alive) { ++dead; continue; }
                bool alone = true;
                for (uint32_t b = others; b; b &= b - 1u) alone &= !meta[__ffs((int)b) - 1].alive;
                float leaf = LK_WIN;
                if (!alone) {
                    if (leaf_q) {
                        const float *z = leaf_q + 3 * (mine + j);
                        leaf = fmaxf(z[0], fmaxf(z[1], z[2]));
                    } else {
                        leaf = best_in[mine + j];
                    }
                }
                worst = fminf(worst, leaf);
            }
            val = dead ? (float)(-2 - dead) - penalty : worst;
        }
    }
    if (par_state != nullptr) {
        float best = fmaxf(val, __shfl_xor(val, 1, 64));
        best = fmaxf(best, __shfl_xor(best, 2, 64));
        if (in && a == 0) best_out[(size_t)row * P + pi] = fold ? best : 0.0f;
    } else if (in && a < 3) {
        q[3 * (size_t)row + a] = !served ? -1.0f : fold ? val : fb_q[3 * (size_t)row + a];
    }
}

// ------------------------------------------------------------------------------------------
// the playout opponent of the pit (snake_engine.arena.Playout, snk_pit_playout_values): flat Monte-Carlo over the scripted policy.
// include/snake_engine.h states the policy, tests/playout_ref.py restates it in plain Python.  Every unblocked move a of a row
// (slot g, snake s) is played out P times for T ticks on copies of the game: clone c = (row * 3 + a) * P + p is slot c of the
// sub-engine.  k_clone, the step kernels and k_pit_script do the copying, the ticks and the plain scores, launched through their
// entry points.  What is new:
//   k_play_plan   a thread per clone: its source slot, whether it is played at all (the pair in range, s alive, two or more
//                 snakes alive, the move not blocked), and the S pairs (c, t) the script kernel scores on it before every tick --
//                 (-1, -1) for a clone that is not played, which the script kernel scores without walking anything
//   k_play_pick   a thread per clone, before each tick: settles the clone when s died in the tick before or stands alone, else
//                 writes the clone's flag for the step and its dense moves -- s's own move a at tick 0, otherwise each alive
//                 snake's playout move from its three plain scores and one Philox draw
//   k_play_fold   a quad of lanes per row, lane a sums the values of its P clones into the score of move a
// Every cell of every array has one writer per launch, nothing is read back, there are no atomics and no LDS, and all per-thread
// state is scalar.  A clone that is not played holds a copy of slot 0 (the clone launch's size is fixed on the host) and is never
// read; a clone that is settled is not stepped again.  Every slot and clone index is compared with its engine's n_slots first.
// ------------------------------------------------------------------------------------------
#define PL_MAX_PLAYOUTS 64
#define PL_MAX_HORIZON 64
#define PL_MAX_EXPLORE 256
#define PL_TAG 0x504C4159u                       // counter word 3 of every playout draw
#define PL_SKIP (-2)                             // a clone's fate: not played
#define PL_RUN (-1)                              //                 still running; 0 .. 2T: its value

// scratch, in int32 elements from its start; every part starts at a multiple of four elements (16 bytes); n = 3 * P * m clones
struct PlayScratch {
    long fb_q;          // float[m][3]       the plain scores of the rows themselves
    long src;           // int32[n]          a clone's source slot (slot 0 for a clone that is not played)
    long fate;          // int32[n]          PL_SKIP, PL_RUN or the clone's value
    long active;        // uint8[n]          a clone's flag for the step
    long moves;         // uint8[n][S]
    long pairs;         // int32[n * S][2]   the fixed list (clone, snake) the script kernel scores before every tick
    long q;             // float[n * S][3]   the tick's plain scores
    long total;
};

static PlayScratch play_scratch(long m, int S, int P)
{
    auto up4 = [](long v) { return (v + 3) / 4 * 4; };
    PlayScratch Z;
    const long n = m * 3 * P;
    long at = 0;
    Z.fb_q = at;    at += up4(3 * m);
    Z.src = at;     at += up4(n);
    Z.fate = at;    at += up4(n);
    Z.active = at;  at += up4((n + 3) / 4);
    Z.moves = at;   at += up4((n * S + 3) / 4);
    Z.pairs = at;   at += up4(2 * n * S);
    Z.q = at;       at += up4(3 * n * S);
    Z.total = at;
    return Z;
}

// the value of a clone whose alive bits after the step of tick i are `bits`: i when s is dead, 2T when s stands alone, else PL_RUN
__device__ static inline int play_settle(uint32_t bits, int s, int i, int T)
{
    if (!((bits >> s) & 1u)) return i;
    return (bits & ~(1u << s)) ? PL_RUN : 2 * T;
}

// thread c < n is clone c: playout c % P of move (c / P) % 3 of row c / (3 * P)
__global__ __launch_bounds__(CMP_THREADS) void k_play_plan(const uint8_t *__restrict__ state, Layout L, int n_slots, int sub_slots,
                                                          const int32_t *__restrict__ pairs, int n, int P,
                                                          const float *__restrict__ fb_q, int32_t *__restrict__ src,
                                                          int32_t *__restrict__ fate, uint8_t *__restrict__ active,
                                                          uint8_t *__restrict__ moves, int32_t *__restrict__ cl_pairs)
{
    const int c = blockIdx.x * CMP_THREADS + threadIdx.x;
    if (c >= n) return;
    const int row = c / (3 * P), a = (c - row * 3 * P) / P;
    const int g = pairs[2 * (size_t)row], s = pairs[2 * (size_t)row + 1];
    bool play = false;
    if (g >= 0 && g < n_slots && s >= 0 && s < L.S && c < sub_slots) {
        const uint32_t bits = slot_alive_bits(state, L, g);
        play = ((bits >> s) & 1u) && __popc(bits) >= 2 && fb_q[3 * (size_t)row + a] != -1.0f;
    }
    src[c] = play ? g : 0;
    fate[c] = play ? PL_RUN : PL_SKIP;
    active[c] = 0;
    for (int t = 0; t < L.S; ++t) {
        const size_t at = (size_t)c * L.S + t;
        moves[at] = 1;
        cl_pairs[2 * at] = play ? c : -1;
        cl_pairs[2 * at + 1] = play ? t : -1;
    }
}

// thread c < n is clone c before the step of tick `tick`; cq holds the plain scores of every (clone, snake) as the clone stands.
// A clone that is not running is not stepped.  A running one is settled when s died in the step before or stands alone; otherwise
// s makes move a at tick 0, and every other alive snake -- s too from tick 1 on -- its playout move: the move k_pit_moves picks
// from its three scores, or, when (r[0] & 255) < eps, the (r[1] % open)-th of its unblocked moves in ascending order
__global__ __launch_bounds__(CMP_THREADS) void k_play_pick(const uint8_t *__restrict__ sub_state, Layout L, int n, int P, int T, int tick,
                                                          int eps, uint32_t k0, uint32_t k1, const int32_t *__restrict__ pairs,
                                                          const float *__restrict__ cq, int32_t *__restrict__ fate,
                                                          uint8_t *__restrict__ active, uint8_t *__restrict__ moves)
{
    const int c = blockIdx.x * CMP_THREADS + threadIdx.x;
    if (c >= n) return;
    if (fate[c] != PL_RUN) { active[c] = 0; return; }
    const int row = c / (3 * P), a = (c - row * 3 * P) / P, p = c - (row * 3 + a) * P;
    const int g = pairs[2 * (size_t)row], s = pairs[2 * (size_t)row + 1];          // in range: the plan played the clone
    const uint32_t bits = slot_alive_bits(sub_state, L, c);                        // c < the sub-engine's n_slots, as above
    if (tick > 0) {
        const int v = play_settle(bits, s, tick - 1, T);
        if (v != PL_RUN) { fate[c] = v; active[c] = 0; return; }
    }
    active[c] = 1;
    for (int t = 0; t < L.S; ++t) {
        int mv = 1;
        if ((bits >> t) & 1u) {
            if (tick == 0 && t == s) {
                mv = a;
            } else {
                const float *z = cq + 3 * ((size_t)c * L.S + t);
                const float q0 = z[0], q1 = z[1], q2 = z[2];
                mv = q0 > q1 ? (q0 > q2 ? 0 : 2) : (q1 > q2 ? 1 : 2);
                const int o0 = q0 != -1.0f, o1 = q1 != -1.0f, open = o0 + o1 + (q2 != -1.0f);
                uint32_t r[4];
                philox4x32((uint32_t)g, (uint32_t)(s | a << 4 | t << 8), (uint32_t)(p | tick << 8), PL_TAG, k0, k1, r);
                if ((int)(r[0] & 255u) < eps && open > 0) {
                    const int k = (int)(r[1] % (uint32_t)open);
                    mv = (o0 && k == 0) ? 0 : (o1 && k == o0) ? 1 : 2;
                }
            }
        }
        moves[(size_t)c * L.S + t] = (uint8_t)mv;
    }
}

// a quad of lanes per row, lane a < 3 scores move a: the row's plain score when its clones were not played (a dead or out-of-range
// pair, fewer than two snakes alive, or the move blocked: -1), else 4 * (the sum of its P clones' values) + (the other moves whose
// plain score is smaller).  A clone still running after the last step is worth T - 1 when s died in it, 2T when s is left alone, T
// otherwise
__global__ __launch_bounds__(CMP_THREADS) void k_play_fold(const uint8_t *__restrict__ sub_state, Layout L, int m, int P, int T,
                                                          const int32_t *__restrict__ pairs, const float *__restrict__ fb_q,
                                                          const int32_t *__restrict__ fate, float *__restrict__ q)
{
    const int t = blockIdx.x * CMP_THREADS + threadIdx.x;
    const int row = t >> 2, a = t & 3;
    if (row >= m || a >= 3) return;
    const int s = pairs[2 * (size_t)row + 1];
    const int base = (row * 3 + a) * P;
    const float z0 = fb_q[3 * (size_t)row], z1 = fb_q[3 * (size_t)row + 1], z2 = fb_q[3 * (size_t)row + 2];
    const float mine = a == 0 ? z0 : a == 1 ? z1 : z2;
    float out = mine;
    if (fate[base] != PL_SKIP) {
        int sum = 0;
        for (int p = 0; p < P; ++p) {
            int v = fate[base + p];
            if (v == PL_RUN) {
                v = play_settle(slot_alive_bits(sub_state, L, base + p), s, T - 1, T);
                if (v == PL_RUN) v = T;
            }
            sum += v;
        }
        const int below = (a != 0 && z0 < mine) + (a != 1 && z1 < mine) + (a != 2 && z2 < mine);
        out = (float)(4 * sum + below);
    }
    q[3 * (size_t)row + a] = out;
}

// ------------------------------------------------------------------------------------------
// replays of chosen games of a pit match (snake_engine.replay.Replay): the two boards Game.tic(show=True) appends per tick
// (Game.draw game.py:281-300, called at game.py:140-141 and 194-195) for a list of recorded slots, drawn into a log in HBM.
// One wavefront per recorded game.  Lane s holds snake s: where its head is drawn, the length it is sorted by, and the run of
// ring entries that are its body.  The board is built in the wave's own LDS in three phases ordered by GAME_SYNC -- food (or
// zeros), heads, bodies -- and stored as dwords plus at most three tail bytes, so the stride padding is never written.
// Heads: sorted() by length is stable over a list in id order (game.py:287), so of the heads on one cell the largest (length, id)
// is drawn last; here the lanes that lose that comparison do not write, and the cell has one writer.  Bodies of different snakes
// share no cell (both would be dead) and a doubled tail writes one value twice.  Every ring walk is bounded by the ring's size
// and every cell index is compared with NC before it indexes the board, whatever the record holds.
// ------------------------------------------------------------------------------------------
#define REC_CELLS ((SNK_MAX_CELLS + 15) / 16 * 16)

__device__ static inline void rec_draw_snakes(int8_t *board, const uint8_t *rec, const Layout &L, int lane, int head, int len_sort,
                                              int first, int cnt)
{
    bool beaten = false;                                  // game.py:287-291: the last head drawn on a cell stays
    for (int o = 0; o < SNK_MAX_SNAKES; ++o) {
        const int ho = __shfl(head, o, 64), lo = __shfl(len_sort, o, 64);
        if (o != lane && ho == head && (lo > len_sort || (lo == len_sort && o > lane))) beaten = true;
    }
    if (head >= 0 && !beaten) board[head] = (int8_t)(-(lane + 1));
    GAME_SYNC();
    for (int s = 0; s < L.S; ++s) {                       // game.py:292-294: the bodies, over the heads
        const int first_s = __shfl(first, s, 64);
        int cnt_s = __shfl(cnt, s, 64);
        cnt_s = cnt_s < L.cap ? cnt_s : L.cap;
        for (int k = lane; k < cnt_s; k += 64) {
            const int c = script_ring_cell(rec, L, s, first_s + k);
            if (c < L.NC) board[c] = (int8_t)(s + 1);
        }
    }
    GAME_SYNC();
}

__device__ static inline void rec_store(const int8_t *board, int8_t *out, int NC, int lane)
{
    for (int j = lane; j < NC / 4; j += 64) ((uint32_t *)out)[j] = ((const uint32_t *)board)[j];
    const int c = (NC & ~3) + lane;
    if (c < NC) out[c] = board[c];
}

// before the step: the snakes of the mid-tick board (game.py:90-127, drawn at :140-141)
__global__ __launch_bounds__(BLOCK_THREADS) void k_pit_record_moves(const uint8_t *__restrict__ state, Layout L, int n_slots,
                                                                   const uint8_t *__restrict__ live, const int32_t *__restrict__ slots,
                                                                   int r, const uint8_t *__restrict__ moves, int8_t *__restrict__ frames,
                                                                   int fstride)
{
    __shared__ __align__(16) int8_t sboard[WAVES_PER_BLOCK][REC_CELLS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * WAVES_PER_BLOCK + wv;
    if (i >= r) return;                                   // whole wavefronts leave: nothing below waits for another wave
    const int slot = slots[i];
    if (slot < 0 || slot >= n_slots || !live[slot]) return;
    int8_t *board = sboard[wv];
    const uint8_t *rec = state + (size_t)slot * L.stride;
    const SnakeMeta *meta = (const SnakeMeta *)(rec + L.meta_off);
    const uint64_t *food = (const uint64_t *)(rec + L.food_off);
    const bool act = lane < L.S;
    SnakeMeta m = {0, 0, 0, 0, 0};
    int mv = 1;
    if (act) { m = meta[lane]; mv = moves[(size_t)slot * L.S + lane]; }
    const bool alive = act && m.alive && m.len >= 1;
    const bool moved = __popcll(__ballot(alive)) >= 2;    // k_step: a game with fewer than two snakes alive stands still
    int head = -1, len_sort = 0, first = 0, cnt = 0;
    if (alive) {
        const int hc = script_ring_cell(rec, L, lane, m.tail + m.len - 1);
        len_sort = m.len;
        cnt = m.len - 1;
        if (moved) {
            const int d = (mv + m.dir + 3) & 3;           // game.py:92
            int y = hc / L.W, x = hc - y * L.W;
            y += (d == 2) - (d == 0);
            x += (d == 1) - (d == 3);
            const bool oob = (y < 0) | (y >= L.H) | (x < 0) | (x >= L.W);
            head = oob ? -1 : y * L.W + x;
            first = m.tail + 1;                           // the tail node is popped, the old head joins the body
        } else {
            head = hc < L.NC ? hc : -1;
            first = m.tail;
        }
    }
    const bool hasfood = moved && head >= 0 && food_bit(food, head);
    bool eats = hasfood;                                  // game.py:121-127: the first snake in list order on a food cell eats
    for (int o = 0; o < SNK_MAX_SNAKES; ++o) {
        const int ho = __shfl(head, o, 64), fo = __shfl((int)hasfood, o, 64);
        if (o < lane && fo && ho == head) eats = false;
    }
    len_sort += eats;
    for (int j = lane; j < fstride / 4; j += 64) ((uint32_t *)board)[j] = 0u;
    GAME_SYNC();
    rec_draw_snakes(board, rec, L, lane, head, len_sort, first, cnt);
    rec_store(board, frames + (size_t)(2 * i) * fstride, L.NC, lane);
}

// after the step: the food into the mid-tick board (game.py:129-138), and the post-tick board (game.py:194-195)
__global__ __launch_bounds__(BLOCK_THREADS) void k_pit_record_boards(const uint8_t *__restrict__ state, Layout L, int n_slots,
                                                                    const uint8_t *__restrict__ live, const int32_t *__restrict__ slots,
                                                                    int r, int8_t *__restrict__ frames, int fstride)
{
    __shared__ __align__(16) int8_t sboard[WAVES_PER_BLOCK][REC_CELLS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * WAVES_PER_BLOCK + wv;
    if (i >= r) return;
    const int slot = slots[i];
    if (slot < 0 || slot >= n_slots || !live[slot]) return;
    int8_t *board = sboard[wv];
    const uint8_t *rec = state + (size_t)slot * L.stride;
    const SnakeMeta *meta = (const SnakeMeta *)(rec + L.meta_off);
    const uint64_t *food = (const uint64_t *)(rec + L.food_off);
    const int NC = L.NC;
    for (int c = lane; c < fstride; c += 64) board[c] = (int8_t)((c < NC && food_bit(food, c)) ? 9 : 0);      // game.py:284-285
    GAME_SYNC();
    SnakeMeta m = {0, 0, 0, 0, 0};
    if (lane < L.S) m = meta[lane];
    int head = -1, len_sort = 0, first = 0, cnt = 0;
    if (lane < L.S && m.alive && m.len >= 1) {
        const int hc = script_ring_cell(rec, L, lane, m.tail + m.len - 1);
        head = hc < NC ? hc : -1;
        len_sort = m.len;
        first = m.tail;
        cnt = m.len - 1;
    }
    rec_draw_snakes(board, rec, L, lane, head, len_sort, first, cnt);
    int8_t *mid = frames + (size_t)(2 * i) * fstride;
    rec_store(board, mid + fstride, NC, lane);
    for (int j = lane; j < NC / 4; j += 64) {             // a cell of the mid-tick board that shows a snake keeps it
        uint32_t v = ((const uint32_t *)mid)[j];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (((v >> (8 * b)) & 0xFFu) == 0u && food_bit(food, 4 * j + b)) v |= 9u << (8 * b);
        ((uint32_t *)mid)[j] = v;
    }
    const int c = (NC & ~3) + lane;
    if (c < NC && mid[c] == 0 && food_bit(food, c)) mid[c] = 9;
}

// ------------------------------------------------------------------------------------------
// the tally of a pit match (snake_engine.tally.Tally): what the tick about to be played does to every seat -- Game.tic's move, eat
// and death phases (game.py:90-165) restated for one tick from the pre-step records and the dense moves, without changing them.
// One wavefront per game, lane s holds snake s; a game is handled when its live flag is set and at least two snakes are alive,
// which is when k_step / k_step_quad move it.  The cross-snake rules (who eats, who loses a head-on) are __shfl over the lanes.
// The body test needs no board: the S new heads sit in registers, the lanes stride over each snake's ring run after the tail is
// popped (old head included; a doubled tail keeps its cell, game.py:354-356) and note per head whether a cell equals it, then one
// ballot per snake.  Every ring walk is bounded by the ring's size and every cell is compared with NC.  Lane s alone writes the
// four cells [g][s]; a snake that lives keeps its fate and died cells.  No LDS, no atomics.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK_THREADS) void k_pit_tally(const uint8_t *__restrict__ state, Layout L, const uint8_t *__restrict__ live,
                                                            int n, const uint8_t *__restrict__ moves, int turn, int health_dec,
                                                            int32_t *__restrict__ fate, int32_t *__restrict__ died,
                                                            int32_t *__restrict__ eaten, int32_t *__restrict__ length)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * WAVES_PER_BLOCK + wv;
    if (g >= n || !live[g]) return;                       // whole wavefronts leave: nothing below waits for another wave
    const uint8_t *rec = state + (size_t)g * L.stride;
    const SnakeMeta *meta = (const SnakeMeta *)(rec + L.meta_off);
    const uint64_t *food = (const uint64_t *)(rec + L.food_off);
    const bool act = lane < L.S;
    SnakeMeta m = {0, 0, 0, 0, 0};
    int mv = 1;
    if (act) { m = meta[lane]; mv = moves[(size_t)g * L.S + lane]; }
    const bool alive = act && m.alive && m.len >= 1;
    if (__popcll(__ballot(alive)) < 2) return;            // k_step: a game with fewer than two snakes alive stands still
    int head = -1, first = 0, cnt = 0;
    if (alive) {
        const int hc = script_ring_cell(rec, L, lane, m.tail + m.len - 1);
        const int d = (mv + m.dir + 3) & 3;               // game.py:92
        int y = hc / L.W, x = hc - y * L.W;
        y += (d == 2) - (d == 0);
        x += (d == 1) - (d == 3);
        const bool oob = (y < 0) | (y >= L.H) | (x < 0) | (x >= L.W);
        head = oob ? -1 : y * L.W + x;                    // -1: off board
        first = m.tail + 1;                               // the tail node is popped, the old head joins the body
        cnt = m.len - 1;
    }
    const bool hasfood = head >= 0 && food_bit(food, head);
    bool eats = hasfood;                                  // game.py:121-127: the first snake in list order on a food cell eats
    int heads[SNK_MAX_SNAKES];
#pragma unroll
    for (int o = 0; o < SNK_MAX_SNAKES; ++o) {
        heads[o] = __shfl(head, o, 64);
        const int fo = __shfl((int)hasfood, o, 64);
        if (o < lane && fo && heads[o] == head) eats = false;
    }
    const int len1 = m.len + (int)eats;                   // game.py:126, Snake.grow
    const int health1 = eats ? 100 : (int16_t)(m.health - health_dec);     // game.py:117-118, 125
    uint32_t hit = 0u;                                    // bit o: this lane met a body cell that is snake o's new head
    for (int s = 0; s < L.S; ++s) {
        const int first_s = __shfl(first, s, 64);
        int cnt_s = __shfl(cnt, s, 64);
        cnt_s = cnt_s < L.cap ? cnt_s : L.cap;
        for (int k = lane; k < cnt_s; k += 64) {
            const int c = script_ring_cell(rec, L, s, first_s + k);
            if (c < L.NC) {
#pragma unroll
                for (int o = 0; o < SNK_MAX_SNAKES; ++o) hit |= (uint32_t)(c == heads[o]) << o;
            }
        }
    }
    bool body = false;
#pragma unroll
    for (int o = 0; o < SNK_MAX_SNAKES; ++o) {
        const bool any = __ballot((hit >> o) & 1u) != 0ull;
        if (o == lane) body = any;
    }
    bool shared = false, lose = false;                    // game.py:156-161, the lengths after the eat phase
#pragma unroll
    for (int o = 0; o < SNK_MAX_SNAKES; ++o) {
        const int lo = __shfl(len1, o, 64);
        if (o != lane && heads[o] >= 0 && heads[o] == head) {
            shared = true;
            if (len1 <= lo) lose = true;
        }
    }
    if (!alive) return;
    int code = 0;                                         // game.py:147-165, an if/elif chain
    if (head < 0) code = 1;
    else if (body) code = 2;
    else if (shared) { if (lose) code = 3; }              // a head-on survivor skips the starvation test
    else if (health1 <= 0) code = 4;
    const size_t at = (size_t)g * L.S + lane;
    if (eats) eaten[at] += 1;
    length[at] = len1;
    if (code) { fate[at] = code; died[at] = turn; }
}

// ------------------------------------------------------------------------------------------ C ABI
// square boards of 5x5 (the eight standard start cells are distinct from there on, game.py:25-29) to 19x19 (SNK_MAX_CELLS);
// the reference's observation is a rot90 of a (2H-1)x(2W-1) canvas, so only square boards batch (game.py:257)
static bool supported_board(int H, int W) { return H == W && H >= 5 && H * W <= SNK_MAX_CELLS; }

#define DISPATCH_BOARD(L, CALL)                                                 \
    do {                                                                        \
        if ((L).H == 11) { constexpr int BH = 11, BW = 11; CALL; }              \
        else if ((L).H == 7) { constexpr int BH = 7, BW = 7; CALL; }            \
        else if ((L).H == 19) { constexpr int BH = 19, BW = 19; CALL; }         \
        else if ((L).NC <= 255) { constexpr int BH = 0, BW = 0; CALL; }         \
        else { constexpr int BH = -1, BW = -1; CALL; }                          \
    } while (0)

// the same for the kernels templated on the 64-bit words of a board plane (Layout::FW): k_pit_script, k_pit_territory
#define DISPATCH_FW(L, CALL)                                                    \
    do {                                                                        \
        if ((L).FW == 1) { constexpr int FW = 1; CALL; }                        \
        else if ((L).FW == 2) { constexpr int FW = 2; CALL; }                   \
        else { constexpr int FW = 6; CALL; }                                    \
    } while (0)

extern "C" int snk_engine_create(snk_engine **out, int n_slots, int H, int W, int S, int health_dec,
                                 double food_spawn_chance, uint64_t seed, int device)
{
    SNK_REQUIRE(out != nullptr, "snk_engine_create: out is NULL");
    SNK_REQUIRE(supported_board(H, W), "snk_engine_create: unsupported board %dx%d (square boards from 5x5 to 19x19)", H, W);
    SNK_REQUIRE(S >= 2 && S <= SNK_MAX_SNAKES, "snk_engine_create: snake count %d outside 2..8", S);
    SNK_REQUIRE(n_slots > 0, "snk_engine_create: n_slots must be positive");
    SNK_CHECK_HIP(hipSetDevice(device));
    snk_engine *e = new snk_engine();
    e->L = make_layout(H, W, S);
    e->n_slots = n_slots;
    e->health_dec = health_dec;
    e->food_chance = food_spawn_chance;
    e->seed = seed;
    e->next_uid = 1;
    e->device = device;
    e->d_state = nullptr;
    e->d_scratch64 = nullptr;
    hipError_t err = hipMalloc((void **)&e->d_state, (size_t)n_slots * e->L.stride);
    if (err == hipSuccess) err = hipMalloc((void **)&e->d_scratch64, 8 * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMemset(e->d_state, 0, (size_t)n_slots * e->L.stride);
    if (err != hipSuccess) {
        snk_set_error("snk_engine_create: device allocation of %zu bytes failed: %s", (size_t)n_slots * e->L.stride, hipGetErrorString(err));
        if (e->d_state) (void)hipFree(e->d_state);
        if (e->d_scratch64) (void)hipFree(e->d_scratch64);
        delete e;
        return -2;
    }
    *out = e;
    return 0;
}

extern "C" int snk_engine_destroy(snk_engine *e)
{
    if (!e) return 0;
    (void)hipFree(e->d_state);
    (void)hipFree(e->d_scratch64);
    delete e;
    return 0;
}

extern "C" int snk_engine_info(const snk_engine *e, int *n_slots, int *H, int *W, int *S, int *slot_bytes)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_info: engine is NULL");
    if (n_slots) *n_slots = e->n_slots;
    if (H) *H = e->L.H;
    if (W) *W = e->L.W;
    if (S) *S = e->L.S;
    if (slot_bytes) *slot_bytes = e->L.stride;
    return 0;
}

extern "C" int snk_engine_raw(const snk_engine *e, void **d_base, int *slot_bytes)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_raw: engine is NULL");
    if (d_base) *d_base = e->d_state;
    if (slot_bytes) *slot_bytes = e->L.stride;
    return 0;
}

extern "C" int snk_engine_set_params(snk_engine *e, int health_dec, double food_spawn_chance)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_set_params: engine is NULL");
    e->health_dec = health_dec;
    e->food_chance = food_spawn_chance;
    return 0;
}

static inline int wave_grid(int n) { return (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK; }

extern "C" int snk_engine_reset(snk_engine *e, const int32_t *d_slots, int n, const uint8_t *d_init_tape, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_reset: engine is NULL");
    SNK_REQUIRE(n >= 0 && (d_slots || n <= e->n_slots), "snk_engine_reset: n=%d exceeds %d slots", n, e->n_slots);
    if (n == 0) return 0;
    const Layout L = e->L;
    const size_t lds = (size_t)WAVES_PER_BLOCK * lds_per_wave(L);
    const uint32_t uid_base = e->next_uid;
    e->next_uid += (uint32_t)n;
    DISPATCH_BOARD(L, (k_reset<BH, BW><<<wave_grid(n), BLOCK_THREADS, lds, (hipStream_t)stream>>>(
        e->d_state, L, d_slots, n, d_init_tape, uid_base, (uint32_t)e->seed, (uint32_t)(e->seed >> 32))));
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_engine_clone(const snk_engine *src, const int32_t *d_src_slots, int n, snk_engine *dst,
                                const int32_t *d_dst_slots, int fanout, void *stream)
{
    SNK_REQUIRE(src && dst, "snk_engine_clone: engine is NULL");
    SNK_REQUIRE(src->L.H == dst->L.H && src->L.W == dst->L.W && src->L.S == dst->L.S, "snk_engine_clone: geometry mismatch");
    SNK_REQUIRE(fanout >= 1, "snk_engine_clone: fanout must be >= 1");
    SNK_REQUIRE(n >= 0 && (d_src_slots || n <= src->n_slots), "snk_engine_clone: n=%d exceeds the source's %d slots", n, src->n_slots);
    SNK_REQUIRE(d_dst_slots || (long long)n * fanout <= dst->n_slots, "snk_engine_clone: %lld copies exceed the destination's %d slots",
                (long long)n * fanout, dst->n_slots);
    if (n == 0) return 0;
    k_clone<<<wave_grid(n), BLOCK_THREADS, 0, (hipStream_t)stream>>>(src->d_state, dst->d_state, src->L, d_src_slots, n, d_dst_slots, fanout);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

static int step_launch(snk_engine *e, const int32_t *d_slots, int n, const uint8_t *d_moves, const int16_t *d_spawn_tape,
                       uint8_t *d_done, int16_t *d_spawned, uint64_t *d_empty, const uint8_t *d_active, void *stream,
                       const int32_t *d_skip = nullptr)
{
    const Layout L = e->L;
    // four games per wavefront where the per-game LDS is small (11x11, 7x7), one per wavefront on 19x19
#define STEP_ARGS e->d_state, L, d_slots, n, d_moves, d_spawn_tape, d_done, d_spawned, d_empty, e->health_dec, e->food_chance, \
                  (uint32_t)e->seed, (uint32_t)(e->seed >> 32), d_active, d_skip
    static const bool wide = getenv("SNK_STEP_FORM") && !strcmp(getenv("SNK_STEP_FORM"), "wide");   // A/B: the lane-group kernel
    if (L.S <= 4 && L.NC <= 255 && !wide) {               // a quad per game, sixteen games per wavefront
        const size_t lds = (size_t)WAVES_PER_BLOCK * 16 * lds_per_game_quad(L);
        const int grid = (n + WAVES_PER_BLOCK * 16 - 1) / (WAVES_PER_BLOCK * 16);
        if (L.H == 11 && L.W == 11 && L.S == 4) k_step_quad<11, 11, 4><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else if (L.H == 7 && L.W == 7 && L.S == 2) k_step_quad<7, 7, 2><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else k_step_quad<0, 0, 0><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
    } else if (L.H <= 11) {
        const size_t lds = (size_t)WAVES_PER_BLOCK * 4 * lds_per_wave(L);
        const int grid = (n + WAVES_PER_BLOCK * 4 - 1) / (WAVES_PER_BLOCK * 4);
        if (L.H == 11 && L.S == 4) k_step<11, 11, 16, 4><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else if (L.H == 11) k_step<11, 11, 16><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else if (L.H == 7) k_step<7, 7, 16><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else k_step<0, 0, 16><<<grid, BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
    } else {
        const size_t lds = (size_t)WAVES_PER_BLOCK * lds_per_wave(L);
        if (L.H == 19) k_step<19, 19, 64><<<wave_grid(n), BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else if (L.NC <= 255) k_step<0, 0, 64><<<wave_grid(n), BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
        else k_step<-1, -1, 64><<<wave_grid(n), BLOCK_THREADS, lds, (hipStream_t)stream>>>(STEP_ARGS);
    }
#undef STEP_ARGS
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_engine_step(snk_engine *e, const int32_t *d_slots, int n, const uint8_t *d_moves,
                               const int16_t *d_spawn_tape, uint8_t *d_done, int16_t *d_spawned,
                               uint64_t *d_empty, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_step: engine is NULL");
    SNK_REQUIRE(n >= 0 && (d_slots || n <= e->n_slots), "snk_engine_step: n=%d exceeds %d slots", n, e->n_slots);
    if (n == 0) return 0;
    SNK_REQUIRE(d_moves != nullptr, "snk_engine_step: d_moves is NULL");
    return step_launch(e, d_slots, n, d_moves, d_spawn_tape, d_done, d_spawned, d_empty, nullptr, stream);
}

extern "C" int snk_engine_step_active(snk_engine *e, const uint8_t *d_active, int n, const uint8_t *d_moves, uint8_t *d_done,
                                      const int32_t *d_skip, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_step_active: engine is NULL");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_engine_step_active: n=%d exceeds %d slots", n, e->n_slots);
    if (n == 0) return 0;
    SNK_REQUIRE(d_moves != nullptr && d_active != nullptr, "snk_engine_step_active: NULL argument");
    return step_launch(e, nullptr, n, d_moves, nullptr, d_done, nullptr, nullptr, d_active, stream, d_skip);
}

extern "C" int snk_engine_step_active_tape(snk_engine *e, const uint8_t *d_active, int n, const uint8_t *d_moves,
                                           const int16_t *d_spawn_tape, uint8_t *d_done, const int32_t *d_skip, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_step_active_tape: engine is NULL");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_engine_step_active_tape: n=%d exceeds %d slots", n, e->n_slots);
    if (n == 0) return 0;
    SNK_REQUIRE(d_moves != nullptr && d_active != nullptr, "snk_engine_step_active_tape: NULL argument");
    return step_launch(e, nullptr, n, d_moves, d_spawn_tape, d_done, nullptr, nullptr, d_active, stream, d_skip);
}

extern "C" int snk_pit_scratch_elems(int n) { return 2 * ((n + PIT_TILE - 1) / PIT_TILE) + 2; }

extern "C" int snk_pit_rows(const snk_engine *e, const uint8_t *d_live, int n, int a_cnt, int32_t *d_pairs, int32_t *d_counts,
                            int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(e && d_counts, "snk_pit_rows: NULL argument");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_rows: n=%d exceeds %d slots", n, e->n_slots);
    SNK_REQUIRE(a_cnt >= 0 && a_cnt <= e->L.S, "snk_pit_rows: a_cnt=%d outside 0..%d", a_cnt, e->L.S);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { SNK_CHECK_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_live && d_pairs && d_scratch, "snk_pit_rows: NULL argument");
    const uint32_t a_bits = (1u << a_cnt) - 1u;
    const int tiles = (n + PIT_TILE - 1) / PIT_TILE;
    k_pit_count<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, a_bits, d_scratch);
    k_pit_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, d_counts);
    k_pit_scatter<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, a_bits, d_scratch, d_counts, d_pairs);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_roots(const snk_engine *e, const uint8_t *d_live, int n, int32_t *d_slots, uint8_t *d_alive, int32_t *d_rank,
                             int32_t *d_count, int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(e && d_count, "snk_pit_roots: NULL argument");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_roots: n=%d exceeds %d slots", n, e->n_slots);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { SNK_CHECK_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_live && d_slots && d_alive && d_rank && d_scratch, "snk_pit_roots: NULL argument");
    const int tiles = (n + PIT_TILE - 1) / PIT_TILE;
    k_pit_roots_count<<<tiles, CMP_THREADS, 0, st>>>(d_live, n, d_scratch);
    k_cmp_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, d_count);
    k_pit_roots_scatter<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, d_scratch, d_slots, d_alive, d_rank);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_verdict(const snk_engine *e, const uint8_t *d_done, const int8_t *d_rewards, int n, int a_cnt, int turn,
                               uint8_t *d_live, int32_t *d_winner, int32_t *d_length, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_pit_verdict: engine is NULL");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_verdict: n=%d exceeds %d slots", n, e->n_slots);
    SNK_REQUIRE(a_cnt >= 0 && a_cnt <= e->L.S, "snk_pit_verdict: a_cnt=%d outside 0..%d", a_cnt, e->L.S);
    if (n == 0) return 0;
    SNK_REQUIRE(d_done && d_rewards && d_live && d_winner && d_length, "snk_pit_verdict: NULL argument");
    k_pit_verdict<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(e->d_state, e->L, d_done, d_rewards, n, (1u << a_cnt) - 1u, turn,
                                                                   d_live, d_winner, d_length);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_owned_scratch_elems(int n, int n_owners)
{
    if (n < 0 || n_owners < 1 || n_owners > SNK_PIT_MAX_OWNERS) return -1;
    return n_owners * ((n + PIT_TILE - 1) / PIT_TILE) + n_owners;
}

extern "C" int snk_pit_rows_owned(const snk_engine *e, const uint8_t *d_live, int n, const uint8_t *d_owner, int n_owners,
                                  int32_t *d_pairs, int32_t *d_counts, int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(e && d_counts, "snk_pit_rows_owned: NULL argument");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_rows_owned: n=%d exceeds %d slots", n, e->n_slots);
    SNK_REQUIRE(n_owners >= 1 && n_owners <= SNK_PIT_MAX_OWNERS, "snk_pit_rows_owned: n_owners=%d outside 1..%d", n_owners,
                SNK_PIT_MAX_OWNERS);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { SNK_CHECK_HIP(hipMemsetAsync(d_counts, 0, n_owners * sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_live && d_owner && d_pairs && d_scratch, "snk_pit_rows_owned: NULL argument");
    const int tiles = (n + PIT_TILE - 1) / PIT_TILE;
    k_lg_count<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, d_owner, n_owners, d_scratch);
    k_lg_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, n_owners, d_counts);
    k_lg_scatter<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, d_owner, n_owners, d_scratch, d_counts, d_pairs);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_verdict_owned(const snk_engine *e, const uint8_t *d_done, const int8_t *d_rewards, int n, const uint8_t *d_owner,
                                     int n_owners, int turn, uint8_t *d_live, int32_t *d_winner, int32_t *d_winner_owner,
                                     int32_t *d_length, void *stream)
{
    SNK_REQUIRE(e != nullptr, "snk_pit_verdict_owned: engine is NULL");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_verdict_owned: n=%d exceeds %d slots", n, e->n_slots);
    SNK_REQUIRE(n_owners >= 1 && n_owners <= SNK_PIT_MAX_OWNERS, "snk_pit_verdict_owned: n_owners=%d outside 1..%d", n_owners,
                SNK_PIT_MAX_OWNERS);
    if (n == 0) return 0;
    SNK_REQUIRE(d_done && d_rewards && d_owner && d_live && d_winner && d_winner_owner && d_length,
                "snk_pit_verdict_owned: NULL argument");
    k_lg_verdict<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(e->d_state, e->L, d_done, d_rewards, n, d_owner, turn, d_live,
                                                                  d_winner, d_winner_owner, d_length);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_roots_owned(const snk_engine *e, const uint8_t *d_live, int n, const uint8_t *d_owner, int n_owners,
                                   uint32_t search_mask, int32_t *d_counts, int32_t *d_slots, uint8_t *d_alive, int32_t *d_rank,
                                   int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(e && d_counts, "snk_pit_roots_owned: NULL argument");
    SNK_REQUIRE(n >= 0 && n <= e->n_slots, "snk_pit_roots_owned: n=%d exceeds %d slots", n, e->n_slots);
    SNK_REQUIRE(n_owners >= 1 && n_owners <= SNK_PIT_MAX_OWNERS, "snk_pit_roots_owned: n_owners=%d outside 1..%d", n_owners,
                SNK_PIT_MAX_OWNERS);
    hipStream_t st = (hipStream_t)stream;
    search_mask &= (1u << n_owners) - 1u;
    if (n == 0 || search_mask == 0u) { SNK_CHECK_HIP(hipMemsetAsync(d_counts, 0, n_owners * sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_live && d_owner && d_slots && d_alive && d_rank && d_scratch, "snk_pit_roots_owned: NULL argument");
    const int tiles = (n + PIT_TILE - 1) / PIT_TILE;
    k_lgs_count<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, d_owner, n_owners, search_mask, d_scratch);
    k_lg_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, n_owners, d_counts);
    k_lgs_scatter<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, e->L, d_live, n, d_owner, n_owners, search_mask, d_scratch, d_counts, d_slots,
                                                 d_alive, d_rank);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the refusals every scripted entry point `fn` shares, in their order: the engine (`engines`: every engine pointer of the call is
// there), the flags, hungry (0..100; 100 where the entry point has none) and m
static int pit_args_ok(const char *fn, bool engines, uint32_t flags, int hungry, int m)
{
    SNK_REQUIRE(engines, "%s: engine is NULL", fn);
    SNK_REQUIRE((flags & ~(uint32_t)(SNK_SCRIPT_SPACE | SNK_SCRIPT_HEADS | SNK_SCRIPT_FOOD)) == 0u, "%s: unknown flag bits in 0x%x", fn,
                flags);
    SNK_REQUIRE(hungry >= 0 && hungry <= 100, "%s: hungry=%d outside 0..100", fn, hungry);
    SNK_REQUIRE(m >= 0, "%s: m=%d", fn, m);
    return 0;
}

// the refusals of one sub-engine of e: there, not e, e's geometry, device and health_dec, no food.  k >= 0: level k of a tree,
// "sub-engine k" in the messages; k < 0: the only one, "the sub-engine"
static int pit_sub_ok(const char *fn, const snk_engine *e, const snk_engine *sub, int k)
{
    char who[32] = "the sub-engine", of[32] = "", both[48] = "the engines";
    if (k >= 0) {
        snprintf(who, sizeof(who), "sub-engine %d", k);
        snprintf(of, sizeof(of), " of %s", who);
        snprintf(both, sizeof(both), "the engine and %s", who);
    }
    SNK_REQUIRE(sub != nullptr, "%s: %s is NULL", fn, who);
    SNK_REQUIRE(sub != e, "%s: %s is the engine itself", fn, who);
    SNK_REQUIRE(e->L.H == sub->L.H && e->L.W == sub->L.W && e->L.S == sub->L.S, "%s: geometry mismatch%s", fn, of);
    SNK_REQUIRE(e->device == sub->device, "%s: %s are on devices %d and %d", fn, both, e->device, sub->device);
    SNK_REQUIRE(sub->food_chance == 0.0 && sub->health_dec == e->health_dec,
                "%s: %s must spawn no food (chance %g) and have the engine's health_dec (%d, not %d)", fn, who, sub->food_chance,
                e->health_dec, sub->health_dec);
    return 0;
}

extern "C" int snk_pit_script_values(const snk_engine *e, const int32_t *d_pairs, int m, uint32_t flags, float *d_q, void *stream)
{
    if (pit_args_ok("snk_pit_script_values", e != nullptr, flags, 100, m)) return -1;
    if (m == 0) return 0;
    SNK_REQUIRE(d_pairs && d_q, "snk_pit_script_values: NULL argument");
    const Layout L = e->L;
    const ScriptMasks K = script_masks(L);
    const int grid = (m + BLOCK_THREADS / 4 - 1) / (BLOCK_THREADS / 4);      // a quad per row
    DISPATCH_FW(L, (k_pit_script<FW><<<grid, BLOCK_THREADS, 0, (hipStream_t)stream>>>(e->d_state, L, e->n_slots, d_pairs, m, flags, K, d_q)));
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_territory_values(const snk_engine *e, const int32_t *d_pairs, int m, uint32_t flags, int hungry, float *d_q,
                                        void *stream)
{
    if (pit_args_ok("snk_pit_territory_values", e != nullptr, flags, hungry, m)) return -1;
    if (m == 0) return 0;
    SNK_REQUIRE(d_pairs && d_q, "snk_pit_territory_values: NULL argument");
    const Layout L = e->L;
    const ScriptMasks K = script_masks(L);
    const int grid = (m + BLOCK_THREADS / 4 - 1) / (BLOCK_THREADS / 4);      // a quad per row
    DISPATCH_FW(L, (k_pit_territory<FW><<<grid, BLOCK_THREADS, 0, (hipStream_t)stream>>>(e->d_state, L, e->n_slots, d_pairs, m, flags,
                                                                                         hungry, K, d_q)));
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the leaf evaluation of the three searching opponents (snk_pit_*_values_leaf): the one-launch scorer of a pair list, the script's
// flood fill or the Voronoi territory.  Both kernels take the same pair lists -- (-1, -1) entries, records a clone and a step have
// just written -- and write the same float32[m][3].
#define LEAF_REFUSAL "%s: leaf=%d, hungry=%d: leaf is SNK_LEAF_SCRIPT with hungry 100 or SNK_LEAF_TERRITORY with hungry 0..100"
static bool leaf_ok(int leaf, int hungry)
{
    return leaf == SNK_LEAF_SCRIPT ? hungry == 100 : leaf == SNK_LEAF_TERRITORY && hungry >= 0 && hungry <= 100;
}

static int leaf_values(const snk_engine *e, const int32_t *d_pairs, int m, uint32_t flags, int leaf, int hungry, float *d_q,
                       void *stream)
{
    return leaf == SNK_LEAF_TERRITORY ? snk_pit_territory_values(e, d_pairs, m, flags, hungry, d_q, stream)
                                      : snk_pit_script_values(e, d_pairs, m, flags, d_q, stream);
}

extern "C" int snk_pit_look_fanout(int S)
{
    if (S < 2 || S > SNK_MAX_SNAKES) return -1;
    return look_pow3(S < 4 ? S : 4);
}

extern "C" int snk_pit_deep_fanout(int S, int depth)
{
    const int F = snk_pit_look_fanout(S);
    if (F < 0 || depth < 1) return -1;
    long p = 1;
    for (int k = 0; k < depth; ++k) { p *= F; if (p > DP_MAX_FANOUT) return -1; }
    return (int)p;
}

extern "C" long snk_pit_deep_scratch_elems(int m, int S, int depth)
{
    const int FD = snk_pit_deep_fanout(S, depth);
    if (m < 0 || FD < 0 || (long long)m * FD > LK_MAX_LEAVES) return -1;
    return deep_scratch(m, S, snk_pit_look_fanout(S), depth).total;
}

extern "C" long snk_pit_look_scratch_elems(int m, int S) { return snk_pit_deep_scratch_elems(m, S, 1); }

// the body of the lookahead (depth 1, one sub-engine) and the deep search, under the name `fn` of the entry point called.  The
// launches of a call, in their order (clone and step through snk_engine_clone and snk_engine_step_active, `leaf` the script or the
// territory kernel through leaf_values):
//   depth 1        k_look_count, k_cmp_scan, k_look_groups, k_look_fan, clone, step, leaf over the m * F leaves, leaf over the m
//                  rows themselves (the fallback), k_deep_reduce
//   depth D >= 2   k_look_count, k_cmp_scan, k_look_groups, leaf over the m rows themselves, D x (k_deep_fan, clone, step),
//                  k_deep_leaves, leaf over the m * F^D leaves, D x k_deep_reduce
// At depth 1 k_look_fan stands for k_deep_fan and k_deep_leaves: the leaf list of a one-level tree needs no stepped level above.
static int search_values(const char *fn, const snk_engine *e, snk_engine *const *subs, int depth, const int32_t *d_pairs, int m,
                         uint32_t flags, int leaf, int hungry, int32_t *d_scratch, float *d_q, void *stream)
{
    SNK_REQUIRE(leaf_ok(leaf, hungry), LEAF_REFUSAL, fn, leaf, hungry);
    if (pit_args_ok(fn, e != nullptr && subs != nullptr, flags, hungry, m)) return -1;
    const Layout L = e->L;
    const int F = snk_pit_look_fanout(L.S), FD = snk_pit_deep_fanout(L.S, depth);
    SNK_REQUIRE(FD > 0, "%s: depth %d with %d snakes (fanout %d) is outside 1 .. the depth at which it reaches %d", fn, depth, L.S, F,
                DP_MAX_FANOUT);
    for (int k = 0; k < depth; ++k) {
        if (pit_sub_ok(fn, e, subs[k], k)) return -1;
        for (int o = 0; o < k; ++o) SNK_REQUIRE(subs[k] != subs[o], "%s: sub-engines %d and %d are the same", fn, o, k);
    }
    if (m == 0) return 0;
    SNK_REQUIRE(d_pairs && d_scratch && d_q, "%s: NULL argument", fn);
    SNK_REQUIRE((long long)m * FD <= LK_MAX_LEAVES, "%s: m=%d rows of fanout %d exceed %d leaves", fn, m, FD, LK_MAX_LEAVES);
    const int need = m < e->n_slots ? m : e->n_slots;
    int n_groups = m;                                     // the groups every level can hold
    {
        long long pw = 1;
        for (int k = 0; k < depth; ++k) {
            pw *= F;
            SNK_REQUIRE(need * pw <= subs[k]->n_slots, "%s: %d groups of fanout %lld exceed sub-engine %d's %d slots", fn, need, pw, k,
                        subs[k]->n_slots);
            if (subs[k]->n_slots / pw < n_groups) n_groups = (int)(subs[k]->n_slots / pw);
        }
    }
    const DeepScratch P = deep_scratch(m, L.S, F, depth);
    int32_t *tile_sums = d_scratch + P.tile_sums, *row_group = d_scratch + P.row_group;
    int32_t *grp_src = d_scratch + P.grp_src, *grp_bits = d_scratch + P.grp_bits, *leaf_pairs = d_scratch + P.leaf_pairs;
    float *leaf_q = (float *)(d_scratch + P.leaf_q), *fb_q = (float *)(d_scratch + P.fb_q);
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (m + PIT_TILE - 1) / PIT_TILE;
    int32_t *count = tile_sums + tiles;
    k_look_count<<<tiles, CMP_THREADS, 0, st>>>(d_pairs, m, tile_sums);
    k_cmp_scan<<<1, CMP_THREADS, 0, st>>>(tile_sums, tiles, count);
    k_look_groups<<<tiles, CMP_THREADS, 0, st>>>(e->d_state, L, e->n_slots, d_pairs, m, tile_sums, count, n_groups, row_group, grp_src,
                                                grp_bits);
    SNK_CHECK_HIP(hipGetLastError());
    int rc = depth > 1 ? leaf_values(e, d_pairs, m, flags, leaf, hungry, fb_q, stream) : 0;
    // level by level: the nodes' flags and moves from the stepped level above, Game.subgame of every node above F times, one tick
    int nodes = n_groups;                                 // of the level above
    for (int k = 0; k < depth && rc == 0; ++k) {
        uint8_t *active = (uint8_t *)(d_scratch + P.active[k]), *moves = (uint8_t *)(d_scratch + P.moves[k]);
        const snk_engine *par = k ? subs[k - 1] : nullptr;
        if (depth == 1)
            k_look_fan<<<(m * F + CMP_THREADS - 1) / CMP_THREADS, CMP_THREADS, 0, st>>>(m, F, L.S, n_groups, d_pairs, row_group, grp_bits,
                                                                                   active, moves, leaf_pairs);
        else
            k_deep_fan<<<(nodes * F + CMP_THREADS - 1) / CMP_THREADS, CMP_THREADS, 0, st>>>(
                nodes * F, F, grp_bits, par ? par->d_state : nullptr, L, par ? par->n_slots : 0,
                k ? (const uint8_t *)(d_scratch + P.active[k - 1]) : nullptr, active, moves);
        SNK_CHECK_HIP(hipGetLastError());
        rc = k ? snk_engine_clone(par, nullptr, nodes, subs[k], nullptr, F, stream)
               : snk_engine_clone(e, grp_src, nodes, subs[k], nullptr, F, stream);
        nodes *= F;
        if (rc == 0) rc = snk_engine_step_active(subs[k], active, nodes, moves, nullptr, nullptr, stream);
    }
    if (rc != 0) return rc;
    if (depth > 1)
        k_deep_leaves<<<(m * FD + CMP_THREADS - 1) / CMP_THREADS, CMP_THREADS, 0, st>>>(
            m, FD, L.S, n_groups, subs[depth - 1]->n_slots, d_pairs, row_group, grp_bits,
            (const uint8_t *)(d_scratch + P.active[depth - 1]), leaf_pairs);
    SNK_CHECK_HIP(hipGetLastError());
    rc = leaf_values(subs[depth - 1], leaf_pairs, m * FD, flags, leaf, hungry, leaf_q, stream);
    if (rc == 0 && depth == 1) rc = leaf_values(e, d_pairs, m, flags, leaf, hungry, fb_q, stream);
    if (rc != 0) return rc;
    // the fold, from the last level up: level k + 1 (subs[k]) into level k
    int per = FD / F;                                     // parents per row: F^k
    for (int k = depth - 1; k >= 0; --k, per /= F) {
        const snk_engine *par = k ? subs[k - 1] : nullptr;
        k_deep_reduce<<<(int)((4LL * m * per + CMP_THREADS - 1) / CMP_THREADS), CMP_THREADS, 0, st>>>(
            par ? par->d_state : nullptr, par ? par->n_slots : 0, k ? (const uint8_t *)(d_scratch + P.active[k - 1]) : nullptr,
            subs[k]->d_state, subs[k]->n_slots, L, m, F, per, n_groups, 32.0f * (float)(depth - 1 - k), d_pairs, row_group, grp_bits,
            k + 1 < depth ? (const float *)(d_scratch + P.best[k]) : nullptr, k + 1 < depth ? nullptr : leaf_q, fb_q,
            k ? (float *)(d_scratch + P.best[k - 1]) : nullptr, d_q);
    }
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_look_values_leaf(const snk_engine *e, snk_engine *sub, const int32_t *d_pairs, int m, uint32_t flags, int leaf,
                                        int hungry, int32_t *d_scratch, float *d_q, void *stream)
{
    return search_values("snk_pit_look_values_leaf", e, sub ? &sub : nullptr, 1, d_pairs, m, flags, leaf, hungry, d_scratch, d_q, stream);
}

extern "C" int snk_pit_look_values(const snk_engine *e, snk_engine *sub, const int32_t *d_pairs, int m, uint32_t flags,
                                   int32_t *d_scratch, float *d_q, void *stream)
{
    return snk_pit_look_values_leaf(e, sub, d_pairs, m, flags, SNK_LEAF_SCRIPT, 100, d_scratch, d_q, stream);
}

extern "C" int snk_pit_deep_values_leaf(const snk_engine *e, snk_engine *const *subs, int depth, const int32_t *d_pairs, int m,
                                        uint32_t flags, int leaf, int hungry, int32_t *d_scratch, float *d_q, void *stream)
{
    return search_values("snk_pit_deep_values_leaf", e, subs, depth, d_pairs, m, flags, leaf, hungry, d_scratch, d_q, stream);
}

extern "C" int snk_pit_deep_values(const snk_engine *e, snk_engine *const *subs, int depth, const int32_t *d_pairs, int m,
                                   uint32_t flags, int32_t *d_scratch, float *d_q, void *stream)
{
    return snk_pit_deep_values_leaf(e, subs, depth, d_pairs, m, flags, SNK_LEAF_SCRIPT, 100, d_scratch, d_q, stream);
}

extern "C" int snk_pit_playout_clones(int P) { return P < 1 || P > PL_MAX_PLAYOUTS ? -1 : 3 * P; }

extern "C" long snk_pit_playout_scratch_elems(int m, int S, int P)
{
    if (m < 0 || S < 2 || S > SNK_MAX_SNAKES || snk_pit_playout_clones(P) < 0 || (long long)m * 3 * P * S > LK_MAX_LEAVES) return -1;
    return play_scratch(m, S, P).total;
}

extern "C" int snk_pit_playout_values_leaf(const snk_engine *e, snk_engine *sub, const int32_t *d_pairs, int m, uint32_t flags, int leaf,
                                           int hungry, int P, int T, int eps, uint64_t seed, int32_t *d_scratch, float *d_q,
                                           void *stream)
{
    SNK_REQUIRE(leaf_ok(leaf, hungry), LEAF_REFUSAL, "snk_pit_playout_values_leaf", leaf, hungry);
    if (pit_args_ok("snk_pit_playout_values_leaf", e != nullptr && sub != nullptr, flags, hungry, m)) return -1;
    SNK_REQUIRE(P >= 1 && P <= PL_MAX_PLAYOUTS, "snk_pit_playout_values_leaf: playouts P=%d outside 1..%d", P, PL_MAX_PLAYOUTS);
    SNK_REQUIRE(T >= 1 && T <= PL_MAX_HORIZON, "snk_pit_playout_values_leaf: horizon T=%d outside 1..%d", T, PL_MAX_HORIZON);
    SNK_REQUIRE(eps >= 0 && eps <= PL_MAX_EXPLORE, "snk_pit_playout_values_leaf: explore eps=%d outside 0..%d", eps, PL_MAX_EXPLORE);
    if (pit_sub_ok("snk_pit_playout_values_leaf", e, sub, -1)) return -1;
    const Layout L = e->L;
    SNK_REQUIRE((long long)m * 3 * P * L.S <= LK_MAX_LEAVES, "snk_pit_playout_values_leaf: m=%d rows of %d clones and %d snakes exceed %d", m,
                3 * P, L.S, LK_MAX_LEAVES);
    SNK_REQUIRE((long long)m * 3 * P <= sub->n_slots, "snk_pit_playout_values_leaf: %d rows of %d clones exceed the sub-engine's %d slots", m,
                3 * P, sub->n_slots);
    if (m == 0) return 0;
    SNK_REQUIRE(d_pairs && d_scratch && d_q, "snk_pit_playout_values_leaf: NULL argument");
    const int n = m * 3 * P;                              // the clones
    const PlayScratch Z = play_scratch(m, L.S, P);
    float *fb_q = (float *)(d_scratch + Z.fb_q), *cq = (float *)(d_scratch + Z.q);
    int32_t *src = d_scratch + Z.src, *fate = d_scratch + Z.fate, *cl_pairs = d_scratch + Z.pairs;
    uint8_t *active = (uint8_t *)(d_scratch + Z.active), *moves = (uint8_t *)(d_scratch + Z.moves);
    hipStream_t st = (hipStream_t)stream;
    const int grid = (n + CMP_THREADS - 1) / CMP_THREADS;
    // the rows' own plain scores (the fallback, the blocked moves, the tie-break), the plan, Game.subgame of every played clone
    int rc = leaf_values(e, d_pairs, m, flags, leaf, hungry, fb_q, stream);
    if (rc != 0) return rc;
    k_play_plan<<<grid, CMP_THREADS, 0, st>>>(e->d_state, L, e->n_slots, sub->n_slots, d_pairs, n, P, fb_q, src, fate, active, moves,
                                             cl_pairs);
    SNK_CHECK_HIP(hipGetLastError());
    rc = snk_engine_clone(e, src, n, sub, nullptr, 1, stream);
    // T ticks: every alive snake's plain scores on every clone, the moves, the step of the clones still running
    for (int i = 0; i < T && rc == 0; ++i) {
        rc = leaf_values(sub, cl_pairs, n * L.S, flags, leaf, hungry, cq, stream);
        if (rc != 0) break;
        k_play_pick<<<grid, CMP_THREADS, 0, st>>>(sub->d_state, L, n, P, T, i, eps, (uint32_t)seed, (uint32_t)(seed >> 32), d_pairs, cq,
                                                 fate, active, moves);
        SNK_CHECK_HIP(hipGetLastError());
        rc = snk_engine_step_active(sub, active, n, moves, nullptr, nullptr, stream);
    }
    if (rc != 0) return rc;
    k_play_fold<<<(4 * m + CMP_THREADS - 1) / CMP_THREADS, CMP_THREADS, 0, st>>>(sub->d_state, L, m, P, T, d_pairs, fb_q, fate, d_q);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_playout_values(const snk_engine *e, snk_engine *sub, const int32_t *d_pairs, int m, uint32_t flags, int P, int T,
                                      int eps, uint64_t seed, int32_t *d_scratch, float *d_q, void *stream)
{
    return snk_pit_playout_values_leaf(e, sub, d_pairs, m, flags, SNK_LEAF_SCRIPT, 100, P, T, eps, seed, d_scratch, d_q, stream);
}

extern "C" int snk_pit_record_stride(int H, int W)
{
    if (!supported_board(H, W)) return -1;
    return align_up(H * W, 16);
}

extern "C" int snk_pit_record_slots(const snk_engine *e, const int32_t *h_slots, int r, int32_t *d_slots, void *stream)
{
    SNK_REQUIRE(r >= 0, "snk_pit_record_slots: r=%d", r);
    if (r == 0) return 0;
    SNK_REQUIRE(e && h_slots && d_slots, "snk_pit_record_slots: NULL argument");
    SNK_REQUIRE(r <= e->n_slots, "snk_pit_record_slots: r=%d exceeds %d slots", r, e->n_slots);
    std::vector<uint8_t> seen((size_t)e->n_slots, 0);
    for (int i = 0; i < r; ++i) {
        const int s = h_slots[i];
        SNK_REQUIRE(s >= 0 && s < e->n_slots, "snk_pit_record_slots: slot %d (entry %d) outside 0..%d", s, i, e->n_slots - 1);
        SNK_REQUIRE(!seen[s], "snk_pit_record_slots: slot %d is listed twice", s);
        seen[s] = 1;
    }
    SNK_CHECK_HIP(hipMemcpyAsync(d_slots, h_slots, (size_t)r * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int snk_pit_record_moves(const snk_engine *e, const uint8_t *d_live, const int32_t *d_slots, int r, const uint8_t *d_moves,
                                    int8_t *d_frames, void *stream)
{
    SNK_REQUIRE(r >= 0, "snk_pit_record_moves: r=%d", r);
    if (r == 0) return 0;
    SNK_REQUIRE(e && d_live && d_slots && d_moves && d_frames, "snk_pit_record_moves: NULL argument");
    SNK_REQUIRE(((uintptr_t)d_frames & 3u) == 0, "snk_pit_record_moves: d_frames is not 4-byte aligned");
    const int fstride = align_up(e->L.NC, 16);
    k_pit_record_moves<<<wave_grid(r), BLOCK_THREADS, 0, (hipStream_t)stream>>>(e->d_state, e->L, e->n_slots, d_live, d_slots, r, d_moves,
                                                                                d_frames, fstride);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_record_boards(const snk_engine *e, const uint8_t *d_live, const int32_t *d_slots, int r, int8_t *d_frames,
                                     void *stream)
{
    SNK_REQUIRE(r >= 0, "snk_pit_record_boards: r=%d", r);
    if (r == 0) return 0;
    SNK_REQUIRE(e && d_live && d_slots && d_frames, "snk_pit_record_boards: NULL argument");
    SNK_REQUIRE(((uintptr_t)d_frames & 3u) == 0, "snk_pit_record_boards: d_frames is not 4-byte aligned");
    const int fstride = align_up(e->L.NC, 16);
    k_pit_record_boards<<<wave_grid(r), BLOCK_THREADS, 0, (hipStream_t)stream>>>(e->d_state, e->L, e->n_slots, d_live, d_slots, r, d_frames,
                                                                                 fstride);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_pit_tally(const snk_engine *e, const uint8_t *d_live, int n, const uint8_t *d_moves, int turn, int32_t *d_fate,
                             int32_t *d_died, int32_t *d_food, int32_t *d_length, void *stream)
{
    SNK_REQUIRE(n >= 0, "snk_pit_tally: n=%d", n);
    if (n == 0) return 0;
    SNK_REQUIRE(e && d_live && d_moves && d_fate && d_died && d_food && d_length, "snk_pit_tally: NULL argument");
    SNK_REQUIRE(n <= e->n_slots, "snk_pit_tally: n=%d exceeds %d slots", n, e->n_slots);
    k_pit_tally<<<wave_grid(n), BLOCK_THREADS, 0, (hipStream_t)stream>>>(e->d_state, e->L, d_live, n, d_moves, turn, e->health_dec, d_fate,
                                                                         d_died, d_food, d_length);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_engine_alive(const snk_engine *e, const int32_t *d_slots, int n, uint8_t *d_alive,
                                int32_t *d_n_alive, void *stream)
{
    SNK_REQUIRE(e != nullptr && d_alive != nullptr, "snk_engine_alive: NULL argument");
    SNK_REQUIRE(n >= 0 && (d_slots || n <= e->n_slots), "snk_engine_alive: n=%d exceeds %d slots", n, e->n_slots);
    if (n == 0) return 0;
    k_alive<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(e->d_state, e->L, d_slots, n, d_alive, d_n_alive);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

static int engine_observe(const snk_engine *e, const int32_t *d_pairs, const int32_t *d_index, int m, int layout, float *d_planes,
                          uint8_t *d_mask, uint64_t *d_key, int legacy_mask, const uint8_t *d_sub_active, uint8_t *d_row_active,
                          void *stream, const uint8_t *d_mirror = nullptr);
extern "C" int snk_engine_observe(const snk_engine *e, const int32_t *d_pairs, int m, int layout,
                                  float *d_planes, uint8_t *d_mask, uint64_t *d_key, int legacy_mask, void *stream)
{
    return engine_observe(e, d_pairs, nullptr, m, layout, d_planes, d_mask, d_key, legacy_mask, nullptr, nullptr, stream);
}
extern "C" int snk_engine_observe_rows(const snk_engine *e, const int32_t *d_pairs, const int32_t *d_index, int m, int layout,
                                       float *d_planes, uint8_t *d_mask, uint64_t *d_key, int legacy_mask,
                                       const uint8_t *d_sub_active, uint8_t *d_row_active, void *stream)
{
    SNK_REQUIRE((d_row_active == nullptr) == (d_sub_active == nullptr), "snk_engine_observe_rows: d_row_active needs d_sub_active (and the other way round)");
    return engine_observe(e, d_pairs, d_index, m, layout, d_planes, d_mask, d_key, legacy_mask, d_sub_active, d_row_active, stream);
}
// the trainer's mirror augmentation (trainer.py:93-97) taken where the observation is encoded: flagged rows come out W-flipped
extern "C" int snk_engine_observe_mirror(const snk_engine *e, const int32_t *d_pairs, const int32_t *d_index, const uint8_t *d_mirror,
                                         int m, int layout, float *d_planes, void *stream)
{
    SNK_REQUIRE(m <= 0 || d_planes != nullptr, "snk_engine_observe_mirror: d_planes is NULL");
    return engine_observe(e, d_pairs, d_index, m, layout, d_planes, nullptr, nullptr, 0, nullptr, nullptr, stream, d_mirror);
}
static int engine_observe(const snk_engine *e, const int32_t *d_pairs, const int32_t *d_index, int m, int layout, float *d_planes,
                          uint8_t *d_mask, uint64_t *d_key, int legacy_mask, const uint8_t *d_sub_active, uint8_t *d_row_active,
                          void *stream, const uint8_t *d_mirror)
{
    SNK_REQUIRE(e != nullptr, "snk_engine_observe: engine is NULL");
    SNK_REQUIRE(layout == SNK_NHWC_F32 || layout == SNK_NCHW_F32 || layout == SNK_NCHW_BF16, "snk_engine_observe: unknown layout %d", layout);
    if (m <= 0) return 0;                               // an empty request is a no-op (its buffers may be NULL)
    SNK_REQUIRE(d_pairs != nullptr, "snk_engine_observe: d_pairs is NULL");
    const Layout L = e->L;
    // Without planes (mask and key only: every rollout state of the MCTS) the work is the per-observation preamble and four
    // observations share a wavefront (11x11, 7x7: their LDS is 1.2 KB each); with planes the kernel is a 5.3 KB store
    // stream per observation and one wavefront per observation keeps more stores in flight (measured: 61 us against 105).
    if (L.H <= 11 && !d_planes) {
        constexpr int WPB = 4;
        const size_t lds = (size_t)WPB * 4 * lds_per_obs(L);
        const int grid = (m + WPB * 4 - 1) / (WPB * 4);
        if (L.H == 11) k_observe<11, 11, 16, WPB><<<grid, WPB * 64, lds, (hipStream_t)stream>>>(e->d_state, L, d_pairs, m, layout, d_planes, d_mask, d_key, legacy_mask, 1, d_index, d_sub_active, d_row_active, d_mirror);
        else if (L.H == 7) k_observe<7, 7, 16, WPB><<<grid, WPB * 64, lds, (hipStream_t)stream>>>(e->d_state, L, d_pairs, m, layout, d_planes, d_mask, d_key, legacy_mask, 1, d_index, d_sub_active, d_row_active, d_mirror);
        else k_observe<0, 0, 16, WPB><<<grid, WPB * 64, lds, (hipStream_t)stream>>>(e->d_state, L, d_pairs, m, layout, d_planes, d_mask, d_key, legacy_mask, 1, d_index, d_sub_active, d_row_active, d_mirror);
    } else {
        const size_t lds = (size_t)WAVES_PER_BLOCK * (!d_planes ? lds_per_obs(L) : layout == SNK_NHWC_F32 ? lds_per_wave_win(L) : lds_per_wave_obs(L));
        // several observations per wavefront once the request fills the chip's wave slots (256 CUs x 32) a few times over
        static const int reps_env = getenv("SNK_OBS_REPS") ? atoi(getenv("SNK_OBS_REPS")) : 0;
        const int reps = reps_env > 0 ? reps_env : (d_planes && m >= 4 * 8192) ? 2 : 1;
        DISPATCH_BOARD(L, (k_observe<BH, BW, 64, WAVES_PER_BLOCK><<<wave_grid((m + reps - 1) / reps), BLOCK_THREADS, lds, (hipStream_t)stream>>>(
            e->d_state, L, d_pairs, m, layout, d_planes, d_mask, d_key, legacy_mask, reps, d_index, d_sub_active, d_row_active, d_mirror)));
    }
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- host views --------------------------------------------------------------------------
static void raw_to_canonical(const Layout &L, const uint8_t *raw, snk_game_state *o)
{
    memset(o, 0, sizeof(*o));
    o->H = L.H; o->W = L.W; o->S = L.S;
    o->uid = *(const uint32_t *)(raw + L.uid_off);
    const SnakeMeta *meta = (const SnakeMeta *)(raw + L.meta_off);
    const uint64_t *food = (const uint64_t *)(raw + L.food_off);
    const uint32_t *cnt = (const uint32_t *)(raw + L.cnt_off);
    const int8_t *rew = (const int8_t *)(raw + L.rew_off);
    for (int s = 0; s < SNK_MAX_SNAKES; ++s)
        for (int k = 0; k < SNK_MAX_NODES; ++k) o->nodes[s][k] = -1;
    for (int s = 0; s < L.S; ++s) {
        o->alive[s] = meta[s].alive;
        o->rewards[s] = rew[s];
        if (!meta[s].alive) continue;
        o->health[s] = meta[s].health;
        o->length[s] = (int16_t)meta[s].len;
        o->dir[s] = meta[s].dir;
        for (int k = 0; k < meta[s].len && k < SNK_MAX_NODES; ++k) {
            const int idx = (meta[s].tail + meta[s].len - 1 - k) & L.cap_mask;      // head first
            const uint8_t *r = raw + s * L.ring_bytes;
            o->nodes[s][k] = (L.cell_bytes == 1) ? (int16_t)r[idx] : (int16_t)((const uint16_t *)r)[idx];
        }
    }
    for (int c = 0; c < L.NC; ++c) o->food[c] = (uint8_t)((food[c >> 6] >> (c & 63)) & 1ull);
    for (int q = 0; q < 6; ++q) o->counters[q] = (int32_t)cnt[q];
}

static int canonical_to_raw(const Layout &L, const snk_game_state *in, uint8_t *raw, int ring_start = 0)
{
    memset(raw, 0, (size_t)L.stride);
    if (in->H != L.H || in->W != L.W || in->S != L.S) return -1;
    SnakeMeta *meta = (SnakeMeta *)(raw + L.meta_off);
    uint64_t *food = (uint64_t *)(raw + L.food_off);
    uint32_t *cnt = (uint32_t *)(raw + L.cnt_off);
    int8_t *rew = (int8_t *)(raw + L.rew_off);
    *(uint32_t *)(raw + L.uid_off) = in->uid;
    for (int s = 0; s < L.S; ++s) {
        rew[s] = in->rewards[s];
        if (!in->alive[s]) continue;
        const int len = in->length[s];
        if (len < 1 || len > L.cap || len > SNK_MAX_NODES) return -2;
        meta[s].alive = 1; meta[s].tail = (uint16_t)(ring_start & L.cap_mask); meta[s].len = (uint16_t)len;
        meta[s].health = in->health[s]; meta[s].dir = in->dir[s];
        uint8_t *r = raw + s * L.ring_bytes;
        for (int k = 0; k < len; ++k) {
            const int cell = in->nodes[s][len - 1 - k];                          // ring index tail + k counts from the tail
            if (cell < 0 || cell >= L.NC) return -3;
            const int at = (ring_start + k) & L.cap_mask;
            if (L.cell_bytes == 1) r[at] = (uint8_t)cell; else ((uint16_t *)r)[at] = (uint16_t)cell;
        }
    }
    for (int c = 0; c < L.NC; ++c) if (in->food[c]) food[c >> 6] |= 1ull << (c & 63);
    for (int q = 0; q < 6; ++q) cnt[q] = (uint32_t)in->counters[q];
    return 0;
}

extern "C" int snk_engine_export_sync(const snk_engine *e, const int32_t *h_slots, int n, snk_game_state *h_out)
{
    SNK_REQUIRE(e != nullptr && h_out != nullptr, "snk_engine_export_sync: NULL argument");
    SNK_REQUIRE(n >= 0 && (h_slots || n <= e->n_slots), "snk_engine_export_sync: n=%d exceeds %d slots", n, e->n_slots);
    const Layout &L = e->L;
    SNK_CHECK_HIP(hipDeviceSynchronize());
    std::vector<uint8_t> raw((size_t)L.stride);
    if (!h_slots) {
        std::vector<uint8_t> all((size_t)n * L.stride);
        if (n) SNK_CHECK_HIP(hipMemcpy(all.data(), e->d_state, all.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) raw_to_canonical(L, all.data() + (size_t)i * L.stride, &h_out[i]);
        return 0;
    }
    for (int i = 0; i < n; ++i) {
        SNK_REQUIRE(h_slots[i] >= 0 && h_slots[i] < e->n_slots, "snk_engine_export_sync: slot %d out of range", h_slots[i]);
        SNK_CHECK_HIP(hipMemcpy(raw.data(), e->d_state + (size_t)h_slots[i] * L.stride, (size_t)L.stride, hipMemcpyDeviceToHost));
        raw_to_canonical(L, raw.data(), &h_out[i]);
    }
    return 0;
}

static int engine_import(snk_engine *e, const int32_t *h_slots, int n, const snk_game_state *h_in, int ring_start);
extern "C" int snk_engine_import_sync(snk_engine *e, const int32_t *h_slots, int n, const snk_game_state *h_in)
{
    return engine_import(e, h_slots, n, h_in, 0);
}
// the same games with every snake's ring laid out from index ring_start on (tail = ring_start mod cap): the state a long game reaches
// -- after cap ticks a live segment straddles the ring's end -- without playing it (tests: the wrap of k_step's and k_observe's ring
// arithmetic).  Export gives back what was imported whatever ring_start is.
extern "C" int snk_engine_import_at_sync(snk_engine *e, const int32_t *h_slots, int n, const snk_game_state *h_in, int ring_start)
{
    SNK_REQUIRE(ring_start >= 0, "snk_engine_import_at_sync: ring_start %d", ring_start);
    return engine_import(e, h_slots, n, h_in, ring_start);
}
static int engine_import(snk_engine *e, const int32_t *h_slots, int n, const snk_game_state *h_in, int ring_start)
{
    SNK_REQUIRE(e != nullptr && h_in != nullptr, "snk_engine_import_sync: NULL argument");
    SNK_REQUIRE(n >= 0 && (h_slots || n <= e->n_slots), "snk_engine_import_sync: n=%d exceeds %d slots", n, e->n_slots);
    const Layout &L = e->L;
    SNK_CHECK_HIP(hipDeviceSynchronize());
    std::vector<uint8_t> raw((size_t)L.stride);
    for (int i = 0; i < n; ++i) {
        const int slot = h_slots ? h_slots[i] : i;
        SNK_REQUIRE(slot >= 0 && slot < e->n_slots, "snk_engine_import_sync: slot %d out of range", slot);
        const int rc = canonical_to_raw(L, &h_in[i], raw.data(), ring_start);
        SNK_REQUIRE(rc == 0, "snk_engine_import_sync: game %d is malformed (code %d)", i, rc);
        SNK_CHECK_HIP(hipMemcpy(e->d_state + (size_t)slot * L.stride, raw.data(), (size_t)L.stride, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int snk_engine_sum_counters_sync(const snk_engine *e, const int32_t *d_slots, int n, int64_t *h_out)
{
    SNK_REQUIRE(e != nullptr && h_out != nullptr, "snk_engine_sum_counters_sync: NULL argument");
    SNK_REQUIRE(n >= 0 && (d_slots || n <= e->n_slots), "snk_engine_sum_counters_sync: n=%d exceeds %d slots", n, e->n_slots);
    SNK_CHECK_HIP(hipMemset(e->d_scratch64, 0, 8 * sizeof(unsigned long long)));
    if (n > 0) {
        int blocks = (n + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        k_sum_counters<<<blocks, 256>>>(e->d_state, e->L, d_slots, n, e->d_scratch64);
        SNK_CHECK_HIP(hipGetLastError());
    }
    unsigned long long tmp[6];
    SNK_CHECK_HIP(hipMemcpy(tmp, e->d_scratch64, sizeof(tmp), hipMemcpyDeviceToHost));
    for (int q = 0; q < 6; ++q) h_out[q] = (int64_t)tmp[q];
    return 0;
}

extern "C" int snk_compact_scratch_elems(int n);

// (slot, snake id) of every alive snake, games in the given order, ids ascending: Game.get_ids over a batch
__global__ void k_ids_from_index(const int32_t *__restrict__ idx, const int32_t *__restrict__ count, const int32_t *__restrict__ slots,
                                 int S, int32_t *__restrict__ pairs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *count) return;
    const int f = idx[i], gi = f / S;
    pairs[2 * i] = slots ? slots[gi] : gi;
    pairs[2 * i + 1] = f - gi * S;
}

extern "C" int snk_engine_ids(const snk_engine *e, const int32_t *d_slots, int n, int32_t *d_pairs, int32_t *d_count,
                              uint8_t *d_alive_scratch, int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(e && d_count, "snk_engine_ids: NULL argument");
    SNK_REQUIRE(n >= 0 && (d_slots || n <= e->n_slots), "snk_engine_ids: n=%d exceeds %d slots", n, e->n_slots);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { SNK_CHECK_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_pairs && d_alive_scratch && d_scratch, "snk_engine_ids: NULL argument");
    const int m = n * e->L.S;
    k_alive<<<(n + 255) / 256, 256, 0, st>>>(e->d_state, e->L, d_slots, n, d_alive_scratch, nullptr);
    int32_t *idx = d_scratch + snk_compact_scratch_elems(m);           // scratch: [tile sums | index list]
    const int tiles = (m + CMP_TILE - 1) / CMP_TILE;
    k_cmp_count<<<tiles, CMP_THREADS, 0, st>>>(d_alive_scratch, m, d_scratch);
    k_cmp_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, d_count);
    k_cmp_scatter<<<tiles, CMP_THREADS, 0, st>>>(d_alive_scratch, m, d_scratch, idx);
    k_ids_from_index<<<(m + 255) / 256, 256, 0, st>>>(idx, d_count, d_slots, e->L.S, d_pairs);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_compact_scratch_elems(int n) { return (n + CMP_TILE - 1) / CMP_TILE + 1; }

extern "C" int snk_compact_flags(const uint8_t *d_flags, int n, int32_t *d_out, int32_t *d_count,
                                 int32_t *d_scratch, void *stream)
{
    SNK_REQUIRE(d_count != nullptr, "snk_compact_flags: d_count is NULL");
    SNK_REQUIRE(n >= 0, "snk_compact_flags: negative n");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { SNK_CHECK_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return 0; }
    SNK_REQUIRE(d_flags && d_out && d_scratch, "snk_compact_flags: NULL argument");
    if (n <= CMP_ONE_MAX) {
        k_cmp_one<<<1, CMP_THREADS, 0, st>>>(d_flags, n, d_out, d_count);
        SNK_CHECK_HIP(hipGetLastError());
        return 0;
    }
    const int tiles = (n + CMP_TILE - 1) / CMP_TILE;
    k_cmp_count<<<tiles, CMP_THREADS, 0, st>>>(d_flags, n, d_scratch);
    k_cmp_scan<<<1, CMP_THREADS, 0, st>>>(d_scratch, tiles, d_count);
    k_cmp_scatter<<<tiles, CMP_THREADS, 0, st>>>(d_flags, n, d_scratch, d_out);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}
