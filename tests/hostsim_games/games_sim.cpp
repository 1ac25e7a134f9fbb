// TEST HARNESS -- the product's supply of games (alpharat_amd/csrc/host_games.h: GameSupply over the seeded maze, start
// cell and cheese samplers) compiled for the CPU and opened to ctypes, one game per call. The header is plain C++, so this
// is the code self-play sessions and matches run, not a restatement. It is NOT a CPU fallback: nothing in alpharat_amd/
// loads this file. games_sweep.cpp is the stand-alone program that runs the same header under the sanitizers.
#include <cstdio>
#include <cstring>

#include "../../alpharat_amd/csrc/host_games.h"

using namespace ar;

extern "C" {

// the fields ArSelfPlayParams and ArMatchParams share, under their names (GameSupply::init reads nothing else)
struct GsParams {
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

// Game `nth` of the run `p` describes. 0: start[2] = the start cells, cheese[hw], cost[hw * 4] (the open maze when the run
// generates none), *index = its game index, *generated = whether the maze is the game's own. -1: the parameters were
// refused, -2: the game could not be made; `err` holds the message.
int gs_make_game(const GsParams* p, uint32_t nth, uint32_t* index, uint8_t* start, uint8_t* cheese, uint8_t* cost, int* generated,
                 char* err, size_t err_cap) {
    std::string msg;
    GameSupply supply;
    HostGame g;
    int rc = 0;
    if (!supply.init(*p, msg)) rc = -1;
    else if (!supply.make_game(supply.index(nth), g, msg)) rc = -2;
    snprintf(err, err_cap, "%s", msg.c_str());
    if (rc != 0) return rc;
    *index = supply.index(nth);
    start[0] = g.p1;
    start[1] = g.p2;
    memcpy(cheese, g.cheese.data(), g.cheese.size());
    const std::vector<uint8_t> c = g.cost.empty() ? open_maze_cost(g.width, g.height) : g.cost;
    memcpy(cost, c.data(), c.size());
    *generated = g.cost.empty() ? 0 : 1;
    return 0;
}

}  // extern "C"
