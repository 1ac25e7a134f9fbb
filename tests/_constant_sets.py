"""Search constants away from the three sets the suite otherwise uses (default, tuned, strong): 24 sets from the grid
c_puct {0, 0.05, 1.5, 8} x fpu_reduction {0, 0.459, 2} x force_k {0, 0.103, 2, 50} x four noise settings, shared by the
device test (test_gpu_offnominal.py) and its CPU twin (test_kernel_logic_cpu.py).

What the values do: c_puct = 0 leaves only q, so every unvisited outcome ties; force_k = 50 forces playouts on every
outcome; epsilon = 1 replaces the prior with the noise; concentration 5.001 puts the gamma sampler at its smallest legal
shape (5.001 / 5) and 400 at shapes up to 200."""
import _oracle as O

C_PUCT = (0.0, 0.05, 1.5, 8.0)
FPU = (0.0, 0.459, 2.0)
FORCE_K = (0.0, 0.103, 2.0, 50.0)
NOISE = ((0.0, 10.83), (1.0, 5.001), (0.6, 400.0), (0.25, 10.83))  # (noise_epsilon, noise_concentration); the first: off

LOW, HIGH = (0.0, 0.0, 0.0), (8.0, 2.0, 50.0)


def _sets():
    out = [(*LOW, *nz) for nz in NOISE] + [(*HIGH, *nz) for nz in NOISE]
    for i in range(16):  # the rest of the grid's values, each with changing partners
        out.append((C_PUCT[i % 4], FPU[(i + i // 4 + 1) % 3], FORCE_K[(i + i // 4 + 1) % 4], *NOISE[(i + i // 8) % 4]))
    return out


SETS = _sets()
IDS = [f"c{c:g}-f{f:g}-k{k:g}-e{e:g}-a{a:g}" for c, f, k, e, a in SETS]


def kwargs(s) -> dict:
    c, f, k, e, a = s
    return dict(c_puct=c, fpu_reduction=f, force_k=k, noise_epsilon=e, noise_concentration=a)


# the shapes of the device test: 5x5, 30 turns, 5 cheese, 120 simulations in batches of 8
W, H, TURNS, CHEESE, SIMS, BATCH = 5, 5, 30, 5, 120, 8
WALLS, MUD = 0.5, 0.3  # the generated mazes: densities that give every game walls and most of them mud


def game(board, i) -> O.Game:
    """game i of a self-play run with seed 0 on the open board or on generated mazes"""
    g = O.Game(W, H, TURNS)
    if board == "maze":
        g.random_maze(WALLS, MUD, True, i)
    return g.random_cheese(CHEESE, True, i)


def rng_seed(i) -> int:
    return 0xA1FA0000 + i
