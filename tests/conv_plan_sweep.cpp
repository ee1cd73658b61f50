// conv_plan_sweep.cpp -- the convolution launch plan (chore_amd/csrc/conv_plan.h) as a stand-alone host program: no HIP, no library.
// tests/test_conv_plan_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it under each switch
// set's environment (the plan's switches are read from the environment, once).
//   conv_plan_sweep           reads "dtype taps B H W Cin Cout traits_bits fill" lines from stdin and prints per line
//                             "family rows nt tps nslot flags class", or "refused: <text>"
//   conv_plan_sweep --grid    every dtype x taps {1, 9} x B {1, 3, 4, 7} x H, W from 8 to 256 (ragged values among them) x Cin, Cout
//                             {32, 64, 128, 256} x every trait combination x fill {0, 128}: prints each distinct
//                             "dtype taps scaled family rows nt tps nslot small_grid cin" once (cin: conv_small / conv_rw only, else 0)
//                             with the number of cases that gave it, and the number of refused cases
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include "../chore_amd/csrc/conv_plan.h"

static ConvTraits traits_of(int bits, int fill) {
    ConvTraits t;
    t.gn = bits & CONV_TRAIT_GN; t.scaled = bits & CONV_TRAIT_SCALED; t.res = bits & CONV_TRAIT_RES; t.res2 = bits & CONV_TRAIT_RES2;
    t.pool = bits & CONV_TRAIT_POOL; t.out = bits & CONV_TRAIT_OUT;
    t.fill = fill;
    return t;
}

int main(int argc, char** argv) {
    const ConvSwitches& sw = conv_switches();
    if (argc > 1 && !strcmp(argv[1], "--grid")) {
        const int Hs[] = {8, 22, 30, 32, 44, 64, 100, 128, 256}, Ws[] = {8, 28, 32, 64, 136, 256}, Cs[] = {32, 64, 128, 256}, Bs[] = {1, 3, 4, 7};
        std::map<std::string, long> seen;
        long refused = 0;
        for (int dtype = 0; dtype < 4; ++dtype)
            for (int taps : {1, 9})
                for (int B : Bs) for (int H : Hs) for (int W : Ws) for (int Cin : Cs) for (int Cout : Cs)
                    for (int bits = 0; bits < 64; ++bits)
                        for (int fill : {0, CONV_MW_FILL_INFER}) {
                            const ConvLaunchPlan p = conv_launch_plan(dtype, taps, B, H, W, Cin, Cout, traits_of(bits, fill), sw);
                            if (p.refuse[0]) { ++refused; continue; }
                            const int cls = conv_profile_class(p, taps, Cin);
                            if (cls < 0 || cls >= CONV_PROFILE_CLASSES || p.small_grid != !!(p.flags & CONV_FLAG_SMALL_GRID)) return 2;
                            char key[96];
                            snprintf(key, sizeof(key), "%d %d %d %d %d %d %d %d %d %d", dtype, taps, !!(bits & CONV_TRAIT_SCALED), p.family, p.rows, p.nt,
                                     p.tps, p.nslot, (int)p.small_grid, p.family == CONV_FAM_SMALL || p.family == CONV_FAM_RW ? Cin : 0);
                            ++seen[key];
                        }
        for (const auto& kv : seen) printf("%s %ld\n", kv.first.c_str(), kv.second);
        printf("refused %ld\n", refused);
        return 0;
    }
    int dtype, taps, B, H, W, Cin, Cout, bits, fill;
    while (scanf("%d %d %d %d %d %d %d %d %d", &dtype, &taps, &B, &H, &W, &Cin, &Cout, &bits, &fill) == 9) {
        const ConvLaunchPlan p = conv_launch_plan(dtype, taps, B, H, W, Cin, Cout, traits_of(bits, fill), sw);
        if (p.refuse[0]) printf("refused: %s\n", p.refuse);
        else printf("%d %d %d %d %d %d %d\n", p.family, p.rows, p.nt, p.tps, p.nslot, p.flags, conv_profile_class(p, taps, Cin));
    }
    return 0;
}
