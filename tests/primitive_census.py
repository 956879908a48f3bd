"""How often do the end-to-end comparisons reach the rarely taken branches of the scalar functions?  For every scene of
tests/test_gpu_parity.py::test_photon_loop_matches_oracle, the oracle follows the test's histories on the CPU and counts (oracle_census) the calls
of meanHG -- the cone mean, used for |g| > 0.95 -- with its two pole folds, of lambertW1 with its series and its asymptotic start, of gexp with its
expansion, and of lnmean with its series.  Prints the table of DESIGN.md section 2 (markdown); run by hand: python tests/primitive_census.py"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COLUMNS = ["meanHG", "forward fold", "backward fold", "lambertW1", "series", "asymptotic", "gexp", "expansion", "lnmean", "series"]


def census(reset=True):
    import oracle_lib as O
    out = (C.c_uint64 * len(COLUMNS))()
    O.lib().oracle_census.restype = None
    O.lib().oracle_census.argtypes = [C.c_void_p, C.c_int]
    O.lib().oracle_census(out, 1 if reset else 0)
    return list(out)


def main():
    import oracle_lib as O
    import test_gpu_parity
    from conftest import ski
    from skirt9_amd.host import Simulation
    scenes = test_gpu_parity.test_photon_loop_matches_oracle.pytestmark[0].args[1]
    print("| scene | histories | " + " | ".join(COLUMNS) + " |")
    print("|---|---|" + "---|" * len(COLUMNS))
    for name, n in scenes:
        sim = Simulation(ski(name), num_packets=n).setup()
        census()
        O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=12345)
        print(f"| {name[:-4]} | {n} | " + " | ".join(str(v) for v in census()) + " |", flush=True)


if __name__ == "__main__":
    main()
