// rr_sample_table.h — the sub-sample table and the regions of a frame: plain host arithmetic, no HIP call.
// Offers: ChaCha12, cell_size_of, rr_sample_table; fill_region, check_region, rr_region_pixel_count.
// Needs:  rr_api_base.h (fail, RR_GUARD_END).

// ---------------------------------------------------------------------------
// the reference's sub-sample table: StdRng::seed_from_u64(0) + shuffle + truncate
// (reference src/raytracing.rs:290-313; rand 0.8: ChaCha12 core, PCG32 seed
// expansion, Fisher-Yates from the back with widening-multiply rejection)
// ---------------------------------------------------------------------------
namespace {

inline uint32_t rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

struct ChaCha12 {
    uint32_t key[8];
    uint64_t counter = 0;
    uint32_t block[16];
    int pos = 16;
    explicit ChaCha12(uint64_t seed) {
        uint64_t state = seed;
        for (int i = 0; i < 8; i++) { // SeedableRng::seed_from_u64
            state = state * 6364136223846793005ull + 11634580027462260723ull;
            uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27);
            uint32_t rot = (uint32_t)(state >> 59);
            key[i] = (xs >> rot) | (xs << ((32u - rot) & 31u));
        }
    }
    void refill() {
        uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                           key[4], key[5], key[6], key[7], (uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
        uint32_t x[16];
        memcpy(x, in, sizeof x);
        auto qr = [&](int a, int b, int c, int d) {
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
        };
        for (int r = 0; r < 6; r++) { // 12 rounds = 6 double rounds
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
        }
        for (int i = 0; i < 16; i++) block[i] = x[i] + in[i];
        counter++;
        pos = 0;
    }
    uint32_t next_u32() { if (pos >= 16) refill(); return block[pos++]; }
    uint32_t below(uint32_t range) { // UniformInt<u32>::sample_single(0, range)
        uint32_t zone = (range << __builtin_clz(range)) - 1u;
        for (;;) {
            uint64_t m = (uint64_t)next_u32() * range;
            if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
        }
    }
};

uint32_t cell_size_of(uint16_t samples) {
    if (samples <= 1) return 1;
    uint16_t v = (uint16_t)(samples + 2);
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p / 2;
}

} // namespace

extern "C" int rr_sample_table(uint16_t samples, uint16_t* xy_out, uint32_t* cell_size_out) try {
    if (!xy_out && samples) return fail(RR_ERR_INVALID_ARGUMENT, "rr_sample_table: xy_out is NULL");
    if (samples > RR_MAX_SAMPLES) return fail(RR_ERR_UNSUPPORTED, "samples %u > %u", (unsigned)samples, RR_MAX_SAMPLES);
    uint32_t cs = cell_size_of(samples);
    std::vector<uint32_t> cells;
    try { cells.resize((size_t)cs * cs); } // 268 MB at the largest cell size: a failure must not cross the C ABI as an exception
    catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "rr_sample_table: no host memory for %u x %u cells", cs, cs); }
    size_t k = 0;
    for (uint32_t xi = 0; xi < cs; xi++)
        for (uint32_t yi = 0; yi < cs; yi++) cells[k++] = xi | (yi << 16);
    ChaCha12 rng(0);
    for (size_t i = cells.size(); i-- > 1;) std::swap(cells[i], cells[rng.below((uint32_t)(i + 1))]);
    for (uint32_t s = 0; s < samples && s < cells.size(); s++) {
        xy_out[2 * s] = (uint16_t)(cells[s] & 0xffffu);
        xy_out[2 * s + 1] = (uint16_t)(cells[s] >> 16);
    }
    if (cell_size_out) *cell_size_out = cs;
    return RR_OK;
} RR_GUARD_END("rr_sample_table")

// xy: the region's pixels in OUTPUT order (tile order, row-major inside the tile; the ABI contract).
// trace_order (optional): a permutation of region indices = the order of the ACCUMULATOR SLOTS, in which
// primary rays are generated: 8x8-pixel blocks inside each tile, so that the 64 lanes of a wave start as one
// compact bundle of rays whatever the tile shape is (32x8 tiles traced in row-major order cost 4 % more than
// 8x8 blocks on sponza_syn) and add to 64 consecutive accumulator words.
static void fill_region(uint32_t w, uint32_t h, const rr_region& rg, std::vector<uint32_t>* xy, std::vector<uint32_t>* trace_order = nullptr) {
    xy->clear();
    if (trace_order) trace_order->clear();
    uint32_t tx = (w + rg.tile_w - 1) / rg.tile_w, ty = (h + rg.tile_h - 1) / rg.tile_h;
    for (uint32_t t = rg.rank; t < tx * ty; t += rg.n_ranks) {
        uint32_t x0 = (t % tx) * rg.tile_w, y0 = (t / tx) * rg.tile_h;
        uint32_t x1 = std::min(x0 + rg.tile_w, w), y1 = std::min(y0 + rg.tile_h, h);
        const uint32_t base = (uint32_t)xy->size(), tw = x1 - x0;
        for (uint32_t y = y0; y < y1; y++)
            for (uint32_t x = x0; x < x1; x++) xy->push_back(x | (y << 16));
        if (trace_order)
            for (uint32_t by = y0; by < y1; by += 8)
                for (uint32_t bx = x0; bx < x1; bx += 8)
                    for (uint32_t y = by; y < std::min(by + 8, y1); y++)
                        for (uint32_t x = bx; x < std::min(bx + 8, x1); x++) trace_order->push_back(base + (y - y0) * tw + (x - x0));
    }
}
static int check_region(uint32_t w, uint32_t h, const rr_region* rg) {
    if (!rg) return fail(RR_ERR_INVALID_ARGUMENT, "region is NULL");
    if (rg->tile_w == 0 || rg->tile_h == 0 || rg->n_ranks == 0 || rg->rank >= rg->n_ranks)
        return fail(RR_ERR_INVALID_ARGUMENT, "bad region: tile %ux%u rank %u of %u", rg->tile_w, rg->tile_h, rg->rank, rg->n_ranks);
    if (w == 0 || h == 0 || w > 65535u || h > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", w, h);
    return RR_OK;
}
extern "C" uint64_t rr_region_pixel_count(uint32_t width, uint32_t height, const rr_region* rg) {
    if (check_region(width, height, rg) != RR_OK) return 0;
    uint32_t tx = (width + rg->tile_w - 1) / rg->tile_w, ty = (height + rg->tile_h - 1) / rg->tile_h;
    uint64_t n = 0;
    for (uint32_t t = rg->rank; t < tx * ty; t += rg->n_ranks) {
        uint32_t x0 = (t % tx) * rg->tile_w, y0 = (t / tx) * rg->tile_h;
        n += (uint64_t)(std::min(x0 + rg->tile_w, width) - x0) * (std::min(y0 + rg->tile_h, height) - y0);
    }
    return n;
}

