// The image plan of tf_fb_calc_slots (transflow_amd/csrc/fb_plan.h) on the CPU, alone: tests/test_fb_plan.py builds
// this with the sanitizers and holds what it prints to the rules.  Every buffer the plan writes is a heap block of
// exactly the capacity it is told, so a write past it is a sanitizer report; a second run over blocks with a guard
// behind them checks the same without the sanitizers.
//
//   fb_plan_host_check CASES
//
// CASES: one case per line,
//   NAME share|no_share|keep SLOTS MAX_PAIRS LIST_CAP prev=a,b,.. next=a,b,.. [expanded=0,1,..] [external=0,1,..]
// LIST_CAP -1: the driver's, 4 * MAX_PAIRS.  Output per case: "NAME list ...", "NAME map (x,y) ...", "NAME runs
// {image0,list0,n} ...", or "NAME error" where the plan does not fit.
#include "../transflow_amd/csrc/fb_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace tf::fb;

static std::vector<int> numbers(const std::string &field)
{
    std::vector<int> v;
    std::stringstream ss(field.substr(field.find('=') + 1));
    for (std::string item; std::getline(ss, item, ',');)
        if (!item.empty())
            v.push_back(atoi(item.c_str()));
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: fb_plan_host_check CASES\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    constexpr int GUARD = 16, MARK = 0x5a5a5a5a;
    for (std::string line; std::getline(in, line);) {
        std::stringstream ss(line);
        std::string name, mode, field;
        int slots = 0, max_pairs = 0, list_cap = 0;
        if (!(ss >> name >> mode >> slots >> max_pairs >> list_cap))
            continue;
        std::vector<int> prev, next, expanded, external;
        while (ss >> field) {
            std::vector<int> &dst = field[0] == 'p' ? prev : field[0] == 'n' ? next : field.compare(0, 3, "exp") == 0 ? expanded : external;
            dst = numbers(field);
        }
        const int n_pairs = (int)prev.size();
        if (next.size() != prev.size() || n_pairs < 1 || n_pairs > max_pairs || slots < 1) {
            fprintf(stderr, "%s: bad case\n", name.c_str());
            return 1;
        }
        std::vector<char> exp_flags(expanded.begin(), expanded.end()), ext_flags(external.begin(), external.end());
        exp_flags.resize((size_t)slots, 0);
        ext_flags.resize((size_t)slots, 0);
        if (list_cap < 0)
            list_cap = 4 * max_pairs;
        const int run_cap = (slots + 1) / 2; // as the handle sizes it
        auto plan = [&](ImagePlan &o) {
            return plan_images(o, slots, n_pairs, prev.data(), next.data(), mode == "keep", mode == "no_share", exp_flags.data(),
                               ext_flags.data());
        };
        // exact blocks: the sanitizers' run
        int *image_of = new int[slots], *list = new int[list_cap ? list_cap : 1];
        ImagePair *map = new ImagePair[n_pairs];
        ImageRun *runs = new ImageRun[run_cap];
        ImagePlan out{image_of, list, list_cap, map, runs, run_cap, 0, 0};
        const bool ok = plan(out);
        // guarded blocks: nothing behind the capacities is touched, and the result is the same
        std::vector<int> g_of((size_t)slots + GUARD, MARK), g_list((size_t)list_cap + GUARD, MARK);
        std::vector<int> g_map(2 * (size_t)n_pairs + GUARD, MARK), g_runs(3 * (size_t)run_cap + GUARD, MARK);
        ImagePlan gout{g_of.data(), g_list.data(), list_cap, reinterpret_cast<ImagePair *>(g_map.data()),
                     reinterpret_cast<ImageRun *>(g_runs.data()), run_cap, 0, 0};
        const bool gok = plan(gout);
        bool same = ok == gok && (!ok || (out.n_list == gout.n_list && out.n_runs == gout.n_runs));
        for (int i = 0; i < GUARD; i++)
            same = same && g_of[(size_t)slots + i] == MARK && g_list[(size_t)list_cap + i] == MARK &&
                   g_map[2 * (size_t)n_pairs + i] == MARK && g_runs[3 * (size_t)run_cap + i] == MARK;
        for (int i = 0; ok && same && i < out.n_list; i++)
            same = list[i] == g_list[(size_t)i];
        if (!same) {
            fprintf(stderr, "%s: the guarded run differs or wrote behind a capacity\n", name.c_str());
            return 1;
        }
        if (!ok) {
            printf("%s error\n", name.c_str());
        } else {
            printf("%s list", name.c_str());
            for (int i = 0; i < out.n_list; i++)
                printf(" %d", list[i]);
            printf("\n%s map", name.c_str());
            for (int i = 0; i < n_pairs; i++)
                printf(" (%d,%d)", map[i].x, map[i].y);
            printf("\n%s runs", name.c_str());
            for (int i = 0; i < out.n_runs; i++)
                printf(" {%d,%d,%d}", runs[i].image0, runs[i].list0, runs[i].n);
            printf("\n");
        }
        delete[] image_of;
        delete[] list;
        delete[] map;
        delete[] runs;
    }
    return 0;
}
