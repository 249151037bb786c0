// The retrieval launcher's policy (foodrec_amd/csrc/m2d_grouped_policy.h) on a CPU: one case per line of standard input,
//   <name> key=value ...
// over the defaults below (the engine's option defaults, E = 64, split bf16, k = 10, 100 k dishes, a 256-CU part); one line per
// case comes back, "<name> field=value ...".  Plain C++17, no HIP.  tests/test_grouped_policy_cpu.py holds the table.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "m2d_grouped_policy.h"

// m2d_catalogue.h's grouped_tiles_per_stage (64 KiB stages), which that header keeps beside the kernels
static int tiles_per_stage(int E) { return E <= 32 ? 16 : (E == 64 ? 8 : (E == 128 ? 4 : 2)); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string name, tok;
        if (!(is >> name)) continue;
        GroupedPolicyIn in{};
        in.E = 64; in.E8 = 0; in.KR = 0; in.BF16X3 = true; in.HV = false; in.PAD = false; in.k = 10; in.nU = 1; in.tiles = 3125;
        in.num_cu = 256; in.topk_form = 0; in.topk_prune = 1; in.topk_block = 0; in.topk_refine = 1; in.variant = 0;
        in.tiles_per_stage = 0; in.half_blocks = true; in.max_probes = 64; in.repair_cap = 1024;
        while (is >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: bad token %s\n", name.c_str(), tok.c_str()); return 2; }
            const std::string key = tok.substr(0, eq);
            const long long v = atoll(tok.c_str() + eq + 1);
            if (key == "E") in.E = (int)v;
            else if (key == "E8") in.E8 = (int)v;
            else if (key == "KR") in.KR = (int)v;
            else if (key == "BF16X3") in.BF16X3 = v != 0;
            else if (key == "HV") in.HV = v != 0;
            else if (key == "PAD") in.PAD = v != 0;
            else if (key == "k") in.k = (int)v;
            else if (key == "nU") in.nU = v;
            else if (key == "tiles") in.tiles = v;
            else if (key == "num_cu") in.num_cu = (int)v;
            else if (key == "topk_form") in.topk_form = (int)v;
            else if (key == "topk_prune") in.topk_prune = (int)v;
            else if (key == "topk_block") in.topk_block = (int)v;
            else if (key == "topk_refine") in.topk_refine = (int)v;
            else if (key == "variant") in.variant = (int)v;
            else if (key == "half_blocks") in.half_blocks = v != 0;
            else { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), key.c_str()); return 2; }
        }
        if (in.E8 == 0) in.E8 = (in.HV ? 2 * in.E : in.E) / 8;          // as m2d_launch_topk_users passes it (no padded width here)
        if (in.KR == 0) in.KR = in.k <= 10 ? 10 : 16;
        in.tiles_per_stage = tiles_per_stage(in.E8 * 8);
        const GroupedPolicy p = grouped_policy(in);
        printf("%s pipe=%d apx=%d half=%d WV=%d TPS=%d lds=%zu ublocks=%lld nsplit=%d planned=%d ext=%d sorted=%d pmode=%d nprobe=%d "
               "plan_quads=%d share_thresholds=%d deal_items=%d prog_limit=%d all_patterns=%d cap=%d\n",
               name.c_str(), p.pipe, p.apx, p.half, p.WV, p.TPS, p.lds, (long long)p.ublocks, p.nsplit, p.planned, p.ext, p.sorted, p.pmode,
               p.nprobe, p.plan_quads, p.share_thresholds, p.deal_items, p.prog_limit, p.all_patterns, p.cap);
    }
    // the split-count hook on its own, with the dense launcher's cap and the grouped launcher's
    printf("hook v0=%d v100=%d v103=%d v199=%d v700=%d\n", topk_split_hook(0, 7, 64), topk_split_hook(100, 7, 64), topk_split_hook(103, 7, 64),
           topk_split_hook(199, 7, 64), topk_split_hook(700, 7, 512));
    return 0;
}
