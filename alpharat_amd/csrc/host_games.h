// Host: the supply of games (our own seeded sampler, DESIGN.md "game generation"). Plain C++ on dev_rng.h / dev_engine.h:
// no HIP call, errors through a std::string&, so the CPU harness of tests/hostsim_games compiles it as it stands.
// GameSupply is the one owner of "which game has index i": self-play sessions and matches both draw from it, which is
// what makes game i of a match the game self-play generates for index first_game_index + i.
#pragma once
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "dev_engine.h"

namespace ar {

struct HostRng {  // same generator family as the device stream, host copy for game generation
    Rng r;
    explicit HostRng(uint64_t seed) { rng_seed(r, seed); }
    uint32_t below(uint32_t n) { return rng_below(r, n); }
};

struct HostGame {
    uint8_t width, height;
    uint16_t max_turns, turn;
    uint8_t p1, p2, m1, m2;
    float s1, s2;
    std::vector<uint8_t> cheese;  // [hw]
    uint16_t total_cheese;
    std::vector<uint8_t> cost;    // [hw * 4] this game's generated maze; empty = the run's shared maze
};

// 180-degree-symmetric cheese: shuffle the pair representatives (i < N-1-i, start cells excluded)
// with Fisher-Yates driven by gen_range, take count/2 pairs; an odd count uses the centre cell.
inline bool place_cheese(HostGame& g, uint32_t count, bool symmetric, uint64_t seed, std::string& err) {
    const int n = g.width * g.height;
    g.cheese.assign(n, 0);
    HostRng rng(seed);
    std::vector<int> cand;
    uint32_t need = count;
    if (symmetric) {
        int centre = -1;
        for (int i = 0; i < n; ++i) {
            const int j = n - 1 - i;
            if (i == g.p1 || i == g.p2 || j == g.p1 || j == g.p2) continue;
            if (i < j) cand.push_back(i);
            else if (i == j) centre = i;
        }
        if (need & 1u) {
            if (centre < 0) {
                err = "odd symmetric cheese count needs a free centre cell";
                return false;
            }
            g.cheese[centre] = 1;
            need -= 1;
        }
        if (need / 2 > cand.size()) {
            err = "cheese_count does not fit the board";
            return false;
        }
        for (int i = (int)cand.size() - 1; i >= 1; --i) std::swap(cand[i], cand[rng.below((uint32_t)i + 1)]);
        for (uint32_t k = 0; k < need / 2; ++k) {
            g.cheese[cand[k]] = 1;
            g.cheese[n - 1 - cand[k]] = 1;
        }
    } else {
        for (int i = 0; i < n; ++i)
            if (i != g.p1 && i != g.p2) cand.push_back(i);
        if (need > cand.size()) {
            err = "cheese_count does not fit the board";
            return false;
        }
        for (int i = (int)cand.size() - 1; i >= 1; --i) std::swap(cand[i], cand[rng.below((uint32_t)i + 1)]);
        for (uint32_t k = 0; k < need; ++k) g.cheese[cand[k]] = 1;
    }
    g.total_cheese = (uint16_t)count;
    return true;
}

inline std::vector<uint8_t> open_maze_cost(int w, int h) {
    std::vector<uint8_t> c((size_t)w * h * 4, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint8_t* p = &c[((size_t)y * w + x) * 4];
            p[DIR_UP] = y + 1 < h;
            p[DIR_RIGHT] = x + 1 < w;
            p[DIR_DOWN] = y > 0;
            p[DIR_LEFT] = x > 0;
        }
    return c;
}

// Random walls + mud: the reference delegates to the pyrat-rust engine (absent, own RNG), so this is our
// own generator -- specification in DESIGN.md "game generation", second implementation in
// oracle/pyrat_engine.hpp::make_maze (the two are compared game by game in the parity tests).
inline std::vector<uint8_t> generate_maze(int w, int h, float wall_density, float mud_density, bool symmetric, uint64_t seed) {
    HostRng rng(seed ^ 0x6D617A65ULL);
    const int n = w * h;
    std::vector<std::pair<int, int>> ed;  // (a, b), a < b; per cell: RIGHT then UP
    std::vector<int> right_of(n, -1), up_of(n, -1);
    for (int i = 0; i < n; ++i) {
        if (i % w + 1 < w) {
            right_of[i] = (int)ed.size();
            ed.emplace_back(i, i + 1);
        }
        if (i / w + 1 < h) {
            up_of[i] = (int)ed.size();
            ed.emplace_back(i, i + w);
        }
    }
    const int ne = (int)ed.size();
    std::vector<int> image(ne);
    for (int k = 0; k < ne; ++k) {
        if (!symmetric) {
            image[k] = k;
            continue;
        }
        const int a = n - 1 - ed[k].second, b = n - 1 - ed[k].first;  // a < b again
        image[k] = b == a + 1 ? right_of[a] : up_of[a];
    }
    std::vector<uint8_t> val(ne, 1);
    const uint32_t wall_thr = (uint32_t)(wall_density * 16777216.0f), mud_thr = (uint32_t)(mud_density * 16777216.0f);
    for (int k = 0; k < ne; ++k)
        if (k <= image[k] && rng.below(1u << 24) < wall_thr) val[k] = val[image[k]] = 0;
    std::vector<int> up(n);
    for (int i = 0; i < n; ++i) up[i] = i;
    int comps = n;
    auto root = [&](int v) {
        while (up[v] != v) v = up[v] = up[up[v]];
        return v;
    };
    auto join = [&](int a, int b) {
        a = root(a);
        b = root(b);
        if (a == b) return;
        if (a < b) up[b] = a;
        else up[a] = b;
        --comps;
    };
    for (int k = 0; k < ne; ++k)
        if (val[k]) join(ed[k].first, ed[k].second);
    std::vector<int> closed;
    for (int k = 0; k < ne; ++k)
        if (k <= image[k] && !val[k]) closed.push_back(k);
    for (int i = (int)closed.size() - 1; i >= 1; --i) std::swap(closed[i], closed[rng.below((uint32_t)i + 1)]);
    for (int k : closed) {
        if (comps == 1) break;
        const int m = image[k];
        if (root(ed[k].first) == root(ed[k].second) && root(ed[m].first) == root(ed[m].second)) continue;
        val[k] = val[m] = 1;
        join(ed[k].first, ed[k].second);
        join(ed[m].first, ed[m].second);
    }
    for (int k = 0; k < ne; ++k)
        if (k <= image[k] && val[k] && rng.below(1u << 24) < mud_thr) val[k] = val[image[k]] = (uint8_t)(2 + rng.below(2));
    std::vector<uint8_t> c((size_t)n * 4, 0);
    for (int k = 0; k < ne; ++k) {
        const int a = ed[k].first, b = ed[k].second;
        const int d = b == a + 1 ? DIR_RIGHT : DIR_UP;
        c[(size_t)a * 4 + d] = val[k];
        c[(size_t)b * 4 + ((d + 2) & 3)] = val[k];
    }
    return c;
}

template <int NW>
void fill_state(const HostGame& g, Board& b, State<NW>& st, uint32_t maze_off) {
    b.width = g.width;
    b.height = g.height;
    b.max_turns = g.max_turns;
    b.total_cheese = g.total_cheese;
    b.maze_off = maze_off;
    for (int k = 0; k < NW; ++k) st.cheese[k] = 0;
    uint16_t rem = 0;
    for (size_t i = 0; i < g.cheese.size(); ++i)
        if (g.cheese[i]) {
            st.cheese[NW == 1 ? 0 : (i >> 6)] |= 1ULL << (i & 63);
            ++rem;
        }
    st.remaining = rem;
    st.s1 = g.s1;
    st.s2 = g.s2;
    st.turn = g.turn;
    st.p1 = g.p1;
    st.p2 = g.p2;
    st.m1 = g.m1;
    st.m2 = g.m2;
}

inline uint64_t entropy_seed() {  // an unseeded run, reference behaviour (selfplay.rs:622, bindings.rs:530-532)
    std::random_device rd;
    const uint64_t hi = rd();
    return (hi << 32) | rd();
}

// The games of a run, by index: game `index` is a function of the fields below alone.
struct GameSupply {
    uint8_t width = 0, height = 0;
    int hw = 0;
    uint16_t max_turns = 0, cheese_count = 0;
    bool cheese_sym = false, random_pos = false, gen_maze = false, maze_sym = true;
    float wall_d = 0.0f, mud_d = 0.0f;
    uint64_t gseed = 0;
    uint32_t first_game_index = 0;

    // `p`: ArSelfPlayParams or ArMatchParams (the fields the two share under the same names). False with `err` set for
    // strings this library does not know and boards it cannot hold.
    template <typename Params>
    bool init(const Params& p, std::string& err) {
        const std::string maze_type = p.maze_type ? p.maze_type : "open", pos = p.positions ? p.positions : "corners";
        if (maze_type != "open" && maze_type != "classic" && maze_type != "random") err = "unknown maze_type: " + maze_type;
        else if (pos != "corners" && pos != "random") err = "unknown positions: " + pos;
        else if (p.width == 0 || p.height == 0 || (int)p.width * p.height > 256) err = "board must have 1..256 cells";
        else err.clear();
        if (!err.empty()) return false;
        width = p.width;
        height = p.height;
        hw = (int)p.width * p.height;
        max_turns = p.max_turns;
        cheese_count = p.cheese_count;
        cheese_sym = p.cheese_symmetric != 0;
        random_pos = pos == "random";
        // "classic" = the engine's default walls and mud (bindings.rs:507 with_classic_maze; taken here as density
        // 0.7 / 0.1, symmetric -- the defaults of the binding's own signature), "random" = the caller's parameters
        gen_maze = maze_type != "open";
        wall_d = maze_type == "classic" ? 0.7f : p.wall_density;
        mud_d = maze_type == "classic" ? 0.1f : p.mud_density;
        maze_sym = maze_type == "classic" ? true : p.maze_symmetric != 0;
        gseed = p.has_seed ? p.game_seed_base : entropy_seed();
        first_game_index = p.first_game_index;
        return true;
    }

    // the index of the run's nth game (wraps in an unbounded session)
    uint32_t index(uint64_t nth) const { return first_game_index + (uint32_t)nth; }

    bool make_game(uint32_t index, HostGame& g, std::string& err) const {
        if (gen_maze) g.cost = generate_maze(width, height, wall_d, mud_d, maze_sym, gseed + index);
        g.width = width;
        g.height = height;
        g.max_turns = max_turns;
        g.turn = 0;
        g.m1 = g.m2 = 0;
        g.s1 = g.s2 = 0.0f;
        g.p1 = 0;
        g.p2 = (uint8_t)(hw - 1);
        if (random_pos) {
            HostRng rng((gseed + index) ^ 0x9E3779B97F4A7C15ULL);
            g.p1 = (uint8_t)rng.below((uint32_t)hw);
            g.p2 = (uint8_t)(hw - 1 - g.p1);
            if (!cheese_sym) g.p2 = (uint8_t)rng.below((uint32_t)hw);
        }
        return place_cheese(g, cheese_count, cheese_sym, gseed + index, err);
    }
};

}  // namespace ar
