"""The register march's band split on the CPU: perc_bands.h is the one copy of
the arithmetic the kernel forms its rows with and the host sizes B's LDS edge
staging by (the staging has no bound check of its own), so its bands must
tile [0, nrows) exactly and the host's tallest band must be the tallest."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, "percolation_amd", "csrc")


def test_band_split_tiles_the_rows(tmp_path):
    exe = str(tmp_path / "march_bands_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "march_bands_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # nrows x Q x ns x weight sets, every band of every cycle
    assert r.stdout.strip().endswith("0 violations"), r.stdout[-2000:]
    assert int(r.stdout.split()[-5]) >= 7 * (1 + 2 + 64 + 256) * (2 + 3 + 4) * 3
