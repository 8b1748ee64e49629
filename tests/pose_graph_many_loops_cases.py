"""Designed graphs with more than LILI_PG_MAX_LOOPS loops (tests/test_pose_graph_many_loops_cpu.py, tests/test_pose_graph_many_loops_gpu.py): the sizes at which the
reduced system over the separators changes hands from the single-workgroup solve (<= 768 unknowns) to the blocked one (tiles of T = api.PG_REDUCED_TILE unknowns).

The graphs are the drifting circuits of tests/pose_graph_cases.py (Cs._looped).  Loops come in bursts of consecutive pairs (a0 + s k, b0 + s k), k = 0 .. count - 1: what
a revisit of a stretch of road produces.  A graph has one separator per distinct loop endpoint and one per multiple of S = LILI_PG_SEGMENT, six reduced unknowns each.

Every case carries `n_sep`, the designed number of separators (the CPU test checks the generator against it).  The function tolerances are set on the MODEL's cost
sequences (seeds 60 .., var 0.1) so that every stop decision is a factor 10 clear of its threshold (Cs.decisions_clear; the CPU test asserts it)."""
from tests import pose_graph_cases as Cs

S = Cs.S
TILE = 96                 # api.PG_REDUCED_TILE
MAX_REDUCED = 768         # api.PG_MAX_REDUCED: the last size of the single-workgroup solve
MAX_LOOPS_EXT = 1024      # api.PG_MAX_LOOPS_EXT


def burst(a0, b0, count, stride=1):
    return [(a0 + stride * k, b0 + stride * k) for k in range(count)]


def separators(case):
    """the separators the library will choose: loop endpoints and multiples of S"""
    n = case["poses"].shape[0]
    ids = set(range(0, n, S))
    for a, b, _, _ in case["loops"]:
        ids.add(a)
        ids.add(b)
    return sorted(ids)


def _case(name, n, seed, pairs, n_sep, ftol, laps=2.0, **kw):
    c = Cs._looped(name, n, seed, pairs, var=0.1, ftol=ftol, laps=laps, **kw)
    c["n_sep"] = n_sep
    return c


def _edge(n_sep):
    """N 600, a burst (330, 20) x m and (599, 0): 2 m + 3 separators (0, 512, 599 and the burst's); an even count takes (560, 512) as well"""
    m = (n_sep - 3) // 2
    pairs = burst(330, 20, m) + [(599, 0)] + ([(560, 512)] if n_sep % 2 == 0 else [])
    return pairs


def tile_edge_sizes():
    """reduced sizes k T - 6, k T, k T + 6 for the smallest k with k T > MAX_REDUCED and for k + 1, as separator counts"""
    k = MAX_REDUCED // TILE + 1
    return [(kk * TILE + d) // 6 for kk in (k, k + 1) for d in (-6, 0, 6)]


# function tolerance per case, read off the model's cost sequence (see the module text)
# (every case ends at its third iteration: the second still drops the cost by 1e-4 .. 1e-2 of it, the third by 1e-9 .. 4e-7, far above the rounding of the sum)
_FTOL = {"loops_33": 1e-6, "loops_64_sep128": 1e-5, "loops_64_sep129": 1e-6, "loops_200": 1e-5, "many_shared_endpoint": 1e-5, "many_adjacent_endpoints": 1e-6}
_FTOL_EDGE = {143: 1e-6, 144: 1e-6, 145: 1e-6, 159: 1e-5, 160: 1e-5, 161: 1e-5}


def designed_cases():
    cs = []
    # the cap alone: 33 loops, 67 separators = 402 unknowns, the single-workgroup solve
    cs.append(_case("loops_33", 200, 60, burst(120, 10, 33), 67, _FTOL["loops_33"], laps=3.0))
    # 128 separators = 768 unknowns: the last size of the single-workgroup solve
    cs.append(_case("loops_64_sep128", 600, 61, burst(330, 20, 62) + [(599, 0), (560, 512)], 128, _FTOL["loops_64_sep128"]))
    # 129 separators = 774 unknowns: the first size of the blocked solve
    cs.append(_case("loops_64_sep129", 600, 62, burst(330, 20, 63) + [(599, 0)], 129, _FTOL["loops_64_sep129"]))
    # the matrix ends 6 short of a tile edge, on it, and 6 past it (the last tile holds one separator), for 9 and for 10 tile columns
    for i, n_sep in enumerate(tile_edge_sizes()):
        cs.append(_case(f"tile_edge_{6 * n_sep}", 600, 70 + i, _edge(n_sep), n_sep, _FTOL_EDGE[n_sep]))
    # stride 2: every burst endpoint is followed by a segment of one node
    cs.append(_case("loops_200", 1500, 63, burst(1001, 101, 200, stride=2), 403, _FTOL["loops_200"], laps=3.0))
    # several loops on one endpoint, the same pair twice and in both directions: a reduced block with several loop blocks, transposed ones among them
    cs.append(_case("many_shared_endpoint", 600, 65, burst(330, 20, 64) + [(450, 20), (470, 20), (490, 25), (330, 20, 0.2), (21, 331), (599, 0)], 134, _FTOL["many_shared_endpoint"]))
    # loops between neighbouring nodes: the block of two adjacent separators carries the chain term and loop blocks, the segment between them is empty
    cs.append(_case("many_adjacent_endpoints", 600, 66, burst(330, 20, 64) + [(450, 451), (452, 451), (500, 498), (599, 0)], 136, _FTOL["many_adjacent_endpoints"]))
    return cs


def loops_1024():
    """the cap: N 8192, two bursts of 512 loops at stride 3; 2060 separators = 12 360 unknowns = 128.75 tiles"""
    c = _case("loops_1024", 8192, 64, burst(4200, 100, 512, stride=3) + burst(6500, 2300, 512, stride=3), 2060, 1e-9, laps=3.0)
    return c
