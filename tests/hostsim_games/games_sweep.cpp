// TEST HARNESS -- a stand-alone sweep of GameSupply::make_game (alpharat_amd/csrc/host_games.h), built with
// -fsanitize=address,undefined (Makefile) and run as a child process by tests/test_game_supply_cpu.py: every board from
// 1x2 to 16x16, the three maze types, both start-cell modes, both cheese symmetries, and the error paths. Exit status 0
// and a line "ok: N games" when every game is well formed and the sanitizers found nothing.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../alpharat_amd/csrc/host_games.h"

using namespace ar;

namespace {

struct Params {  // the fields GameSupply::init reads
    uint8_t width, height;
    uint16_t cheese_count, max_turns;
    int cheese_symmetric;
    const char* maze_type;
    const char* positions;
    float wall_density, mud_density;
    int maze_symmetric, has_seed;
    uint64_t game_seed_base;
    uint32_t first_game_index;
};

[[noreturn]] void die(const Params& p, const char* what, const std::string& msg = "") {
    fprintf(stderr, "games_sweep: %ux%u %s %s sym %d count %u: %s %s\n", p.width, p.height, p.maze_type ? p.maze_type : "-",
            p.positions ? p.positions : "-", p.cheese_symmetric, p.cheese_count, what, msg.c_str());
    exit(1);
}

void expect_error(const Params& p, bool at_init, const std::string& want) {
    GameSupply s;
    HostGame g;
    std::string err;
    const bool ok = s.init(p, err);
    if (at_init ? ok : !ok) die(p, "init", err);
    if (!at_init && s.make_game(s.index(0), g, err)) die(p, "no error, wanted", want);
    if (err != want) die(p, "message", err);
}

}  // namespace

int main() {
    unsigned long games = 0;
    const char* maze_types[3] = {"open", "classic", "random"};
    const char* positions[2] = {"corners", "random"};
    for (int w = 1; w <= 16; ++w)
        for (int h = 1; h <= 16; ++h) {
            const int hw = w * h;
            if (hw < 2) continue;
            for (const char* mt : maze_types)
                for (const char* pos : positions)
                    for (int sym = 0; sym < 2; ++sym) {
                        // an even count that fits beside any two start cells (an odd symmetric one needs the centre free)
                        const Params p = {(uint8_t)w, (uint8_t)h, (uint16_t)(((hw - 2) / 2) & ~1), 30, sym, mt, pos, 0.6f, 0.3f,
                                          (w + h) & 1, 1, 0x1234ULL * (uint64_t)hw, (uint32_t)(0xFFFFFFFEu * (uint32_t)sym)};
                        GameSupply s;
                        std::string err;
                        if (!s.init(p, err)) die(p, "init", err);
                        for (uint64_t nth = 0; nth < 3; ++nth) {  // (with sym the index wraps past 2^32 - 1)
                            HostGame g;
                            if (!s.make_game(s.index(nth), g, err)) die(p, "make_game", err);
                            if (g.p1 >= hw || g.p2 >= hw) die(p, "start cell outside the board");
                            if (sym && g.p2 != hw - 1 - g.p1) die(p, "start cells not symmetric");
                            if ((int)g.cheese.size() != hw) die(p, "cheese size");
                            unsigned n = 0;
                            for (int c = 0; c < hw; ++c) n += g.cheese[c];
                            if (n != p.cheese_count || g.total_cheese != n) die(p, "cheese count");
                            if (g.cheese[g.p1] || g.cheese[g.p2]) die(p, "cheese on a start cell");
                            if (g.cost.size() != (s.gen_maze ? (size_t)hw * 4 : 0u)) die(p, "maze size");
                            State<4> st;
                            Board b;
                            fill_state<4>(g, b, st, 0);
                            if (st.remaining != n) die(p, "fill_state");
                            ++games;
                        }
                    }
        }
    Params e = {4, 4, 3, 30, 1, "open", "corners", 0.0f, 0.0f, 1, 1, 7, 0};
    expect_error(e, false, "odd symmetric cheese count needs a free centre cell");
    e.cheese_count = 16;
    expect_error(e, false, "cheese_count does not fit the board");
    e.cheese_symmetric = 0;
    e.cheese_count = 15;
    expect_error(e, false, "cheese_count does not fit the board");
    e.maze_type = "hexagonal";
    expect_error(e, true, "unknown maze_type: hexagonal");
    e.maze_type = nullptr;
    e.positions = "centre";
    expect_error(e, true, "unknown positions: centre");
    e.positions = nullptr;
    e.width = 17;
    e.height = 16;
    expect_error(e, true, "board must have 1..256 cells");
    e.width = 0;
    expect_error(e, true, "board must have 1..256 cells");
    printf("ok: %lu games\n", games);
    return 0;
}
