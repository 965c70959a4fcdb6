// tests/host/rw_check.hip -- the host side of the random walks without a GPU: RwOptions (app/rw/rw_enactor.hpp) parses the options and
// picks the strategy of AUTO; Pitch, Draw, ChooseUniform, ChooseWeighted and RowHolds (app/rw/rw_functor.hpp) are the __host__
// __device__ functions the kernels walk with.  The draws are the literals tests/test_rw_cpu.py pins; every other expectation follows
// from a formula of the definition.  Built with -Xarch_host -fsanitize=address,undefined by tests/test_rw_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/rw/rw_enactor.hpp>

using namespace gunrock::app::rw;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    RwOptions o;
    // parsing: 1 for a name nobody knows, -1 for a value out of range, a NaN or what no integer holds
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.Set("nope", 1, true) == 1);
    CHECK(o.Set("strategy", 3, true) == -1 && o.Set("strategy", -1, true) == -1 && o.Set("strategy", nan, true) == -1);
    CHECK(o.Set("length", -1, true) == -1 && o.Set("length", 16777216, true) == -1 && o.Set("length", 1e300, true) == -1);
    CHECK(o.Set("seed", -1, true) == -1 && o.Set("seed", 9007199254740992.0, true) == -1 && o.Set("seed", 0.5, true) == -1 && o.Set("seed", -1e300, true) == -1);
    CHECK(o.Set("weighted", 2, true) == -1 && o.Set("weighted", 1, false) == -1 && o.Set("weighted", 0, false) == 0);
    CHECK(o.Set("bias_return", 65536, true) == -1 && o.Set("bias_in", -1, true) == -1 && o.Set("bias_out", nan, true) == -1);
    CHECK(o.Set("tries", 0, true) == -1 && o.Set("tries", 129, true) == -1 && o.Set("visits", 2, true) == -1 && o.Set("visits", -1, true) == -1);
    // a refused value leaves the option as it was: the defaults
    CHECK(o.strategy == RW_AUTO && o.length == 0 && o.seed == 0 && o.weighted == 0 && o.bias_return == 1 && o.bias_in == 1 && o.bias_out == 1 &&
          o.tries == 32 && o.visits == 0 && !o.Biased());
    CHECK(o.Set("length", 16777215, true) == 0 && o.length == kMaxLength && o.Set("seed", 9007199254740991.0, true) == 0 &&
          o.seed == 9007199254740991ull && o.Set("weighted", 1, true) == 0 && o.weighted == 1);
    CHECK(o.Set("bias_return", 65535, true) == 0 && o.Set("bias_in", 0, true) == 0 && o.Set("bias_out", 7, true) == 0);
    CHECK(o.bias_return == 65535 && o.bias_in == 0 && o.bias_out == 7 && o.Biased() && o.MaxBias() == 65535);
    CHECK(o.Set("bias_return", 3, true) == 0 && o.MaxBias() == 7 && o.Set("bias_in", 9, true) == 0 && o.MaxBias() == 9);
    CHECK(o.Set("bias_return", 9, true) == 0 && o.Set("bias_out", 9, true) == 0 && !o.Biased());
    CHECK(o.Set("tries", 1, true) == 0 && o.tries == 1 && o.Set("tries", 128, true) == 0 && o.tries == 128 && o.Set("visits", 1, true) == 0 && o.visits == 1);

    // AUTO on both sides of the threshold; a forced strategy whatever the length
    RwOptions a;
    CHECK(a.Set("length", kTileMinLength - 1, false) == 0 && a.Strategy() == RW_LANE);
    CHECK(a.Set("length", kTileMinLength, false) == 0 && a.Strategy() == RW_TILE);
    CHECK(a.Set("length", 0, false) == 0 && a.Strategy() == RW_LANE && a.Set("length", kMaxLength, false) == 0 && a.Strategy() == RW_TILE);
    CHECK(a.Set("strategy", RW_LANE, false) == 0 && a.Strategy() == RW_LANE && a.Set("length", 0, false) == 0 &&
          a.Set("strategy", RW_TILE, false) == 0 && a.Strategy() == RW_TILE);

    // the pitch: length + 1 entries rounded up to 16
    CHECK(Pitch(0) == 16 && Pitch(14) == 16 && Pitch(15) == 16 && Pitch(16) == 32 && Pitch(31) == 32 && Pitch(32) == 48 && Pitch(48) == 64);
    CHECK(Pitch(kMaxLength) == 16777216);
    for (long long length = 0; length < 100; ++length) CHECK(Pitch(length) % 16 == 0 && Pitch(length) >= length + 1 && Pitch(length) < length + 17);

    // the draws
    const uint64_t r0 = Draw(0, 0, 0, 0), r1 = Draw(1, 2, 3, 4), r2 = Draw(9007199254740991ull, 2147483647ull, 16777215ull, 255),
                   r3 = Draw(20261020, 65, 17, 1);
    CHECK(r0 == 12035550249420947055ull && r1 == 13731179152291499476ull && r2 == 4361106646733862201ull && r3 == 414575086076068509ull);
    // unweighted: k = ((r >> 32) * d) >> 32
    CHECK(ChooseUniform(r0, 7) == 4 && ChooseUniform(r1, 7) == 5 && ChooseUniform(r2, 7) == 1 && ChooseUniform(r3, 7) == 0);
    CHECK(ChooseUniform(r0, 5000) == 3262 && ChooseUniform(r1, 5000) == 3721 && ChooseUniform(r2, 5000) == 1182 && ChooseUniform(r3, 5000) == 112);
    CHECK(ChooseUniform(r0, 1) == 0 && ChooseUniform(~0ull, 2147483647) == 2147483646 && ChooseUniform(0, 2147483647) == 0);
    // weighted: t = (r * T) >> 64, the smallest index whose inclusive prefix exceeds t.  Weights 3, 0, 5, 2: t = 6, 7, 2, 0
    const long long small[4] = {3, 3, 8, 10};
    CHECK(MulHigh(r0, 10) == 6 && MulHigh(r1, 10) == 7 && MulHigh(r2, 10) == 2 && MulHigh(r3, 10) == 0);
    CHECK(ChooseWeighted(r0, small, 4) == 2 && ChooseWeighted(r1, small, 4) == 2 && ChooseWeighted(r2, small, 4) == 0 && ChooseWeighted(r3, small, 4) == 0);
    CHECK(ChooseWeighted(~0ull, small, 4) == 3 && ChooseWeighted(0, small, 4) == 0);
    const long long after_zero[3] = {0, 0, 4};  // a zero-weight entry is never chosen
    CHECK(ChooseWeighted(0, after_zero, 3) == 2 && ChooseWeighted(r1, after_zero, 3) == 2);
    // three entries of weight 2^31 - 1: T = 6442450941 > 2^32, the product needs its high word
    const long long big[3] = {2147483647LL, 4294967294LL, 6442450941LL};
    CHECK(MulHigh(r0, 6442450941ull) == 4203367364ull && MulHigh(r1, 6442450941ull) == 4795558917ull && MulHigh(r2, 6442450941ull) == 1523098900ull &&
          MulHigh(r3, 6442450941ull) == 144788676ull);
    CHECK(ChooseWeighted(r0, big, 3) == 1 && ChooseWeighted(r1, big, 3) == 2 && ChooseWeighted(r2, big, 3) == 0 && ChooseWeighted(r3, big, 3) == 0);
    CHECK(MulHigh(~0ull, ~0ull) == ~0ull - 1 && MulHigh(1ull << 63, 2) == 1 && MulHigh(~0ull, 1) == 0);
    // membership in a sorted row with duplicates
    const int row[6] = {1, 4, 4, 9, 12, 12};
    CHECK(RowHolds(row, 6, 1) && RowHolds(row, 6, 4) && RowHolds(row, 6, 12) && !RowHolds(row, 6, 0) && !RowHolds(row, 6, 5) && !RowHolds(row, 6, 13));
    CHECK(!RowHolds(row, 0, 1) && RowHolds(row + 3, 1, 9) && !RowHolds(row + 3, 1, 4));
    std::puts("rw host checks passed");
    return 0;
}
