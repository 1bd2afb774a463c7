"""The library's one host Gold sequence (csrc/lte_seq_host.cpp: gold_bytes, gold_words), no GPU: tools/lte_seq_check.cpp
built with it under the address and undefined-behaviour sanitizers checks the two output formats against each other
and prints their bits; here the bits are compared with Oracle().sequence_bits, which tests/test_phy_oracle.py pins to
the reference's compiled sequence.c."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEEDS_ASKED = (0, 1, 2**30, 2**31 - 1)
LENGTHS = (1, 31, 32, 33, 48, 1920, 2200)  # word boundaries, the PUCCH word, PBCH's longest, 20 * 110
NOF_CALL_SITE_SEEDS = 8


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("lte_seq") / "lte_seq_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "lte_seq_check.cpp"),
                    os.path.join(ROOT, "srsran_4g_amd", "csrc", "lte_seq_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return [ln.split() for ln in r.stdout.splitlines()]


def test_cases_cover_the_seeds_and_lengths(lines):
    seeds = []
    for seed, _, _, _ in lines:
        if int(seed) not in seeds:
            seeds.append(int(seed))
    assert tuple(seeds[:4]) == SEEDS_ASKED and len(seeds) == 4 + NOF_CALL_SITE_SEEDS, seeds
    assert max(seeds) < 2**31
    assert [(int(s), int(n)) for s, n, _, _ in lines] == [(s, n) for s in seeds for n in LENGTHS]


def test_bits_match_the_oracle(lines):
    ora = Oracle()
    for seed, n, bits, words in lines:
        seed, n = int(seed), int(n)
        want = ora.sequence_bits(seed, n)
        got = np.frombuffer(bits.encode(), np.uint8) - ord("0")
        assert got.size == n and np.array_equal(got, want), (seed, n, np.flatnonzero(got != want)[:8])
        w = np.array([int(words[8 * k: 8 * k + 8], 16) for k in range(len(words) // 8)], np.uint32)
        assert w.size == (n + 31) // 32
        packed = (w[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1
        assert np.array_equal(packed, want), (seed, n)
