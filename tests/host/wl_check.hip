// tests/host/wl_check.hip -- the host side of colour refinement, without a GPU: the 128-bit mix against values computed from its
// formula, the wrapping sum and the cut to sig_bits, the lane / wave / workgroup split of the signature pass, the rung of a
// certificate, the size of the grouping table, and the options with their ranges and ABI codes.  Every expectation follows from a
// formula in app/wl/wl_functor.hpp, wl_enactor.hpp or wl_problem.hpp.  Built with -Xarch_host -fsanitize=address,undefined by
// tests/test_wl_host.py; makes no HIP call.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/wl/wl_enactor.hpp>

using namespace gunrock::app::wl;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// splitmix64's finaliser, written out again
static uint64_t Finalise(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

int main()
{
    // Mix(seed, attempt, colour) = (F(seed ^ F(x)), F(seed ^ F(~x))), x = attempt << 32 | colour
    const uint64_t seeds[] = {0, 1, 0x6772, ~0ull};
    const uint64_t attempts[] = {1, 2, 77, 0xFFFFFFFFull};
    const int colours[] = {0, 1, 64, 2147483647};
    for (uint64_t seed : seeds)
        for (uint64_t attempt : attempts)
            for (int colour : colours) {
                const uint64_t x = (attempt << 32) | static_cast<uint32_t>(colour);
                const Sig s = Mix(seed, attempt, colour);
                CHECK(s.lo == Finalise(seed ^ Finalise(x)) && s.hi == Finalise(seed ^ Finalise(~x)));
            }
    // (two values by hand from the formula: tests/test_wl_host.py compares them with the Python wl_mix too)
    CHECK(Mix(0, 1, 0).lo == 13831967835898817870ull && Mix(0, 1, 0).hi == 9618544736715962354ull);
    CHECK(Mix(0, 1, 0).lo != Mix(0, 2, 0).lo && Mix(0, 1, 0).lo != Mix(0, 1, 1).lo && Mix(1, 1, 0).lo != Mix(0, 1, 0).lo);

    // the sum: 128-bit, wrapping, with the carry from the low word; it commutes
    Sig a{~0ull, 0}, one{1, 0};
    Add(a, one);
    CHECK(a.lo == 0 && a.hi == 1);
    Sig top{~0ull, ~0ull};
    Add(top, one);
    CHECK(top.lo == 0 && top.hi == 0);
    Sig l{0, 0}, r{0, 0};
    for (int i = 0; i < 100; ++i) Add(l, Mix(3, 5, i));
    for (int i = 99; i >= 0; --i) Add(r, Mix(3, 5, i));
    CHECK(l.lo == r.lo && l.hi == r.hi);
    unsigned __int128 wide = 0;
    for (int i = 0; i < 100; ++i) wide += (static_cast<unsigned __int128>(Mix(3, 5, i).hi) << 64) | Mix(3, 5, i).lo;
    CHECK(l.lo == static_cast<uint64_t>(wide) && l.hi == static_cast<uint64_t>(wide >> 64));

    // the cut: the top `bits` bits
    const Sig full{0xFEDCBA9876543210ull, 0x0123456789ABCDEFull};
    CHECK(Truncate(full, 128).lo == full.lo && Truncate(full, 128).hi == full.hi);
    CHECK(Truncate(full, 64).lo == full.hi && Truncate(full, 64).hi == 0);
    CHECK(Truncate(full, 65).lo == 0x02468ACF13579BDFull && Truncate(full, 65).hi == 0);
    CHECK(Truncate(full, 127).lo == 0xFF6E5D4C3B2A1908ull && Truncate(full, 127).hi == 0x0091A2B3C4D5E6F7ull);
    CHECK(Truncate(full, 1).lo == 0 && Truncate(full, 1).hi == 0 && Truncate(full, 2).lo == 0 && Truncate(full, 5).lo == 0);
    CHECK(Truncate(full, 8).lo == 0x01 && Truncate(full, 12).lo == 0x012 && Truncate(full, 63).lo == 0x0091A2B3C4D5E6F7ull && Truncate(full, 63).hi == 0);
    const Sig high{0, 0x8000000000000000ull};
    CHECK(Truncate(high, 1).lo == 1 && Truncate(high, 2).lo == 2 && Truncate(high, 64).lo == high.hi && Truncate(high, 65).hi == 1 && Truncate(high, 65).lo == 0);
    {   // a row of one colour k times: the cut still depends on the colour (the low bits of k m would not, for even k)
        Sig four_a{0, 0}, four_b{0, 0};
        int told = 0;
        for (int attempt = 1; attempt <= 64; ++attempt) {
            four_a = four_b = Sig{0, 0};
            for (int i = 0; i < 4; ++i) Add(four_a, Mix(0, attempt, 5)), Add(four_b, Mix(0, attempt, 9));
            told += Truncate(four_a, 2).lo != Truncate(four_b, 2).lo;
            CHECK((four_a.lo & 3) == 0 && (four_b.lo & 3) == 0);
        }
        CHECK(told >= 32);  // (3/4 of the attempts in the mean)
    }

    // the split of the signature pass: lp's
    CHECK(WL_AUTO == 0 && WL_LANE == 1 && WL_WAVE == 2 && WL_BLOCK == 3 && kLaneMaxRow == 16 && kWaveMaxRow == 4096);
    CHECK(Regime(1, WL_AUTO, 16, 4096) == WL_LANE && Regime(16, WL_AUTO, 16, 4096) == WL_LANE && Regime(17, WL_AUTO, 16, 4096) == WL_WAVE);
    CHECK(Regime(4096, WL_AUTO, 16, 4096) == WL_WAVE && Regime(4097, WL_AUTO, 16, 4096) == WL_BLOCK && Regime(2147483647, WL_AUTO, 16, 4096) == WL_BLOCK);
    CHECK(Regime(1, WL_AUTO, 0, 0) == WL_BLOCK && Regime(1, WL_AUTO, 0, 1) == WL_WAVE);
    for (int strategy = WL_LANE; strategy <= WL_BLOCK; ++strategy) CHECK(Regime(1, strategy, 16, 4096) == strategy && Regime(1 << 20, strategy, 16, 4096) == strategy);

    // the rung of a certificate: both rows in the table, 2 d entries
    CHECK(Rung(1, 1024, 8192) == WL_RUNG_WAVE && Rung(256, 1024, 8192) == WL_RUNG_WAVE && Rung(257, 1024, 8192) == WL_RUNG_BLOCK);
    CHECK(Rung(2048, 1024, 8192) == WL_RUNG_BLOCK && Rung(2049, 1024, 8192) == WL_RUNG_GLOBAL && Rung(2147483647, 1024, 8192) == WL_RUNG_GLOBAL);
    CHECK(Rung(16, 64, 256) == WL_RUNG_WAVE && Rung(17, 64, 256) == WL_RUNG_BLOCK && Rung(64, 64, 256) == WL_RUNG_BLOCK && Rung(65, 64, 256) == WL_RUNG_GLOBAL);
    for (int d = 1; d < 3000; ++d) {  // what a rung holds fits its table twice over
        const int rung = Rung(d, 1024, 8192);
        if (rung != WL_RUNG_GLOBAL) CHECK(gunrock::app::ladder::TableSize(2ll * d, rung == WL_RUNG_WAVE ? 1024 : 8192) >= 4 * d);
        CHECK(Rung(d, 1024, 8192) <= Rung(d + 1, 1024, 8192));
    }

    // the grouping table: the smallest power of two that is at least 2 n, at least 64
    typedef WlProblem<false> Problem;
    CHECK(Problem::TableSlots(1) == 64 && Problem::TableSlots(32) == 64 && Problem::TableSlots(33) == 128 && Problem::TableSlots(65) == 256);
    CHECK(Problem::TableSlots(1 << 20) == (2u << 20) && Problem::TableSlots((1 << 20) + 1) == (4u << 20));
    CHECK(Problem::TableSlots(2147483647LL) == (1ull << 32));  // (held in 64 bits: nothing wraps)

    // the options: 0 taken, -1 out of range, 1 unknown
    WlOptions o;
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.strategy == WL_AUTO && o.lane_max_row == 16 && o.wave_max_row == 4096 && o.max_rounds == -1 && o.max_repairs == 64 && o.history == 0 &&
          o.sig_bits == 128 && o.seed == 0);
    CHECK(o.Set("nope", 1) == 1 && o.Set("", 1) == 1 && o.Set("mode", 0) == 1 && o.Set("nope", nan) == 1);
    CHECK(o.Set("strategy", 4) == -1 && o.Set("strategy", -1) == -1 && o.Set("strategy", nan) == -1 && o.Set("strategy", WL_BLOCK) == 0 &&
          o.strategy == WL_BLOCK && o.Set("strategy", WL_AUTO) == 0);
    CHECK(o.Set("lane_max_row", -1) == -1 && o.Set("lane_max_row", 0) == 0 && o.lane_max_row == 0 && o.Set("lane_max_row", 1e300) == 0 &&
          o.lane_max_row == (1 << 30));
    CHECK(o.Set("wave_max_row", -1) == -1 && o.Set("wave_max_row", nan) == -1 && o.Set("wave_max_row", 7) == 0 && o.wave_max_row == 7);
    CHECK(o.Set("max_rounds", -2) == -1 && o.Set("max_rounds", 1e300) == -1 && o.Set("max_rounds", nan) == -1 && o.max_rounds == -1);
    CHECK(o.Set("max_rounds", 0) == 0 && o.max_rounds == 0 && o.CertifyAll() && o.Set("max_rounds", 1 << 30) == 0 && o.Set("max_rounds", -1) == 0 &&
          !o.CertifyAll());
    CHECK(o.Set("max_repairs", -1) == -1 && o.Set("max_repairs", 2e9) == -1 && o.Set("max_repairs", 0) == 0 && o.max_repairs == 0 &&
          o.Set("max_repairs", 4096) == 0 && o.max_repairs == 4096);
    CHECK(o.Set("sig_bits", 0) == -1 && o.Set("sig_bits", 129) == -1 && o.Set("sig_bits", nan) == -1 && o.sig_bits == 128 && o.Set("sig_bits", 1) == 0 &&
          o.sig_bits == 1 && o.Set("sig_bits", 128) == 0);
    CHECK(o.Set("seed", -1) == -1 && o.Set("seed", 1e300) == -1 && o.Set("seed", nan) == -1 && o.Set("seed", 12345) == 0 && o.seed == 12345 &&
          o.Set("seed", 9007199254740992.0) == 0 && o.seed == (1ull << 53));
    CHECK(o.Set("history", 2) == -1 && o.Set("history", -1) == -1 && o.Set("history", 1) == 0 && o.history == 1);
    // history asks for max_rounds in 1 .. 64 and for (max_rounds + 1) n colours within int32
    CHECK(!o.HistoryValid() && o.Set("max_rounds", 0) == 0 && !o.HistoryValid() && o.Set("max_rounds", 65) == 0 && !o.HistoryValid());
    CHECK(o.Set("max_rounds", 64) == 0 && o.HistoryValid() && o.Set("max_rounds", 1) == 0 && o.HistoryValid());
    CHECK(o.HistoryFits(1073741823) && !o.HistoryFits(1073741824) && o.Set("max_rounds", 64) == 0 && o.HistoryFits(33038209) && !o.HistoryFits(33038210));
    CHECK(o.Set("history", 0) == 0 && o.HistoryValid() && o.HistoryFits(2147483647) && o.Set("max_rounds", -1) == 0);
    // the table's options are the ladder's
    CHECK(o.Set("table_slots", 96) == -1 && o.Set("table_slots", 32) == -1 && o.Set("table_slots", 2048) == -1 && o.Set("table_slots", 64) == 0);
    CHECK(o.Set("block_slots", 128) == -1 && o.Set("block_slots", 16384) == -1 && o.Set("block_slots", 256) == 0);
    CHECK(o.Set("scratch_mib", 0) == -1 && o.Set("scratch_mib", 65537) == -1 && o.Set("scratch_mib", nan) == -1 && o.Set("scratch_mib", 1) == 0);
    CHECK(o.table.table_slots == 64 && o.table.block_slots == 256 && o.table.scratch_mib == 1);
    // which kernels a graph can need, from its longest row
    CHECK(!o.AnyBlock(0) && !o.AnyBlock(16) && o.AnyBlock(17) && !o.AnyGlobal(64) && o.AnyGlobal(65) && o.AnyBlock(65));
    CHECK(o.Set("strategy", WL_AUTO) == 0 && o.Set("lane_max_row", 16) == 0 && o.Set("wave_max_row", 512) == 0);
    CHECK(!o.AnyHub(0) && !o.AnyHub(512) && o.AnyHub(513) && o.Set("strategy", WL_BLOCK) == 0 && o.AnyHub(1) && !o.AnyHub(0) &&
          o.Set("strategy", WL_WAVE) == 0 && !o.AnyHub(1 << 20));
    CHECK(o.Set("strategy", WL_AUTO) == 0 && !o.AnyWave(0) && !o.AnyWave(16) && o.AnyWave(17) && o.AnyWave(1 << 20));
    CHECK(o.Set("wave_max_row", 16) == 0 && !o.AnyWave(1 << 20) && o.Set("strategy", WL_WAVE) == 0 && o.AnyWave(1) && !o.AnyWave(0));
    CHECK(o.Set("strategy", WL_LANE) == 0 && !o.AnyWave(1 << 20) && !o.AnyHub(1 << 20));
    std::puts("wl host checks passed");
    return 0;
}
