"""Writes tests/golden/meshgen_ref/: output files of the REFERENCE's meshGen (its src/meshgen/main_all.cpp compiled
as-is into oracle/_ref/meshGen_ref by `make -C oracle ref`, REFERENCE naming the reference checkout; std-only source, no
stand-ins) for the argument sets of CASES, and gzip-compressed under live/ for the larger argument sets of LIVE_CASES.
Run where the reference checkout exists; the files are data fixtures the twin (fem-shell_amd/host/meshGen) is
byte-compared with on any machine."""
import gzip
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "meshGen_ref")
OUT = os.path.join(ROOT, "tests", "golden", "meshgen_ref")

CASES = {
    "tri_z_uniform": "t 7 5 -1.5 0 2 3 0,1,-1,2 2.5 2 1 z",
    "tri_y_flap_unit": "t 4 9 0 0 0.1 1 2,20,2,2 1 1 0 y",
    "quad_z_testD16": "q 16 16 0 0 10 10 0,0,0,0 300 2 1 z",
    "quad_x_testF_con": "q 3 3 0 0 10 2 1,1,1,1 0.0004 1 1 x",
    "quad_z_noload": "q 5 2 -3 1 7 8.5 -1,21,-1,-1 1e-4 0 1 z",
    "tri_z_thirds": "t 3 3 0 0 1 1 0,0,0,0 1 2 1 z",
}

# tests/test_host_tools.py::test_meshgen_twin_against_the_live_reference_tool: the 64x64 Test-G meshes and more
LIVE_CASES = {
    "tri_z_testG64": "t 64 64 0 0 10 10 0,0,0,0 300 2 1 z",
    "quad_z_testG64": "q 64 64 0 0 10 10 0,0,0,0 300 2 1 z",
    "tri_x_mixed_bc": "t 13 21 0 0 2 3 0,-1,1,-1 5 2 0 x",
    "quad_z_small_load": "q 32 32 0 0 10 2 0,0,0,0 0.0001 2 1 z",
    "tri_z_noload": "t 8 2 0 0 48 12 -1,-1,0,-1 1 0 1 z",
    "tri_y_flap_thirds": "t 10 30 0.05 -0.25 0.15 0.75 2,20,2,2 0.3333333 1 1 y",
}

if __name__ == "__main__":
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ref"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "CASES.txt"), "w") as f:
        for name, args in CASES.items():
            subprocess.check_call([REF] + args.split() + [os.path.join(OUT, name)], stdout=subprocess.DEVNULL)
            f.write("%s: %s\n" % (name, args))
    live = os.path.join(OUT, "live")
    os.makedirs(live, exist_ok=True)
    with open(os.path.join(live, "CASES.txt"), "w") as f, tempfile.TemporaryDirectory() as td:
        for name, args in LIVE_CASES.items():
            subprocess.check_call([REF] + args.split() + [os.path.join(td, name)], stdout=subprocess.DEVNULL)
            for ext in (".xda", "_f"):
                if os.path.exists(os.path.join(td, name + ext)):
                    with open(os.path.join(td, name + ext), "rb") as src:
                        # (mtime 0: the same bytes on every run)
                        with gzip.GzipFile(os.path.join(live, name + ext + ".gz"), "wb", compresslevel=9, mtime=0) as dst:
                            dst.write(src.read())
            f.write("%s: %s\n" % (name, args))
    print("wrote", OUT)
