"""The v2 attention kernels' workgroup order (csrc/attn_work_order.h), checked
exhaustively on the host: a stand-alone C++ program includes the header and
prints the map for every linear block id of every grid below; the properties
are asserted here.

  * the map is a bijection onto nx x gy x gz (every tile is computed exactly
    once, and no index leaves the grid);
  * with G = gy*gz a multiple of 8, a group (head, batch) lands on exactly one
    residue L % 8 (one XCD, one L2), and every residue holds each rank equally
    often (the same multiset of block weights per XCD);
  * within a residue the rank never decreases with L (heaviest first); with
    G % 8 != 0 the same holds over the whole grid.
"""
import collections
import os
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parents[2] / "pipegoose_amd/ops/csrc"

NX = (1, 2, 3, 8, 16)
GYZ = ((4, 2), (16, 8), (3, 1), (5, 3), (2, 4))

PROGRAM = r"""
#include <cstdio>
#include "attn_work_order.h"

int main() {
    const unsigned nxs[] = {%(nx)s};
    const unsigned gyz[][2] = {%(gyz)s};
    for (unsigned nx : nxs) {
        for (const auto& g : gyz) {
            const unsigned total = nx * g[0] * g[1];
            for (unsigned L = 0; L < total; ++L) {
                const AttnWork w = attn_work_order(L, g[0], g[1]);
                std::printf("%%u %%u %%u %%u %%d %%d %%d\n", nx, g[0], g[1], L,
                            w.rank, w.h, w.b);
            }
        }
    }
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def work_map(tmp_path_factory):
    """{(nx, gy, gz): [(rank, h, b) for L in range(nx*gy*gz)]}"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    tmp = tmp_path_factory.mktemp("attn_work_order")
    src = tmp / "work_order_main.cpp"
    src.write_text(PROGRAM % {
        "nx": ", ".join(map(str, NX)),
        "gyz": ", ".join("{%d, %d}" % g for g in GYZ)})
    exe = tmp / "work_order_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                    f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout
    table = collections.defaultdict(list)
    for line in out.splitlines():
        nx, gy, gz, L, rank, h, b = map(int, line.split())
        assert L == len(table[nx, gy, gz])
        table[nx, gy, gz].append((rank, h, b))
    assert set(table) == {(nx, gy, gz) for nx in NX for gy, gz in GYZ}
    return dict(table)


@pytest.mark.parametrize("gyz", GYZ)
@pytest.mark.parametrize("nx", NX)
def test_work_order_is_a_bijection(work_map, nx, gyz):
    gy, gz = gyz
    m = work_map[nx, gy, gz]
    assert len(m) == nx * gy * gz
    assert set(m) == {(r, h, b) for r in range(nx) for h in range(gy)
                      for b in range(gz)}


@pytest.mark.parametrize("gyz", [g for g in GYZ if g[0] * g[1] % 8 == 0])
@pytest.mark.parametrize("nx", NX)
def test_work_order_pins_groups_and_balances_xcds(work_map, nx, gyz):
    gy, gz = gyz
    m = work_map[nx, gy, gz]
    residues = collections.defaultdict(set)      # group -> {L % 8}
    ranks = collections.defaultdict(collections.Counter)  # L % 8 -> rank counts
    for L, (rank, h, b) in enumerate(m):
        residues[h, b].add(L % 8)
        ranks[L % 8][rank] += 1
    assert len(residues) == gy * gz
    assert all(len(r) == 1 for r in residues.values()), residues
    want = collections.Counter({r: gy * gz // 8 for r in range(nx)})
    assert sorted(ranks) == list(range(8))
    assert all(c == want for c in ranks.values()), ranks


@pytest.mark.parametrize("gyz", GYZ)
@pytest.mark.parametrize("nx", NX)
def test_work_order_is_heaviest_first(work_map, nx, gyz):
    gy, gz = gyz
    m = work_map[nx, gy, gz]
    # issue order within an XCD; over the whole grid when groups are not pinned
    step = 8 if gy * gz % 8 == 0 else 1
    for r in range(step):
        seq = [rank for rank, _, _ in m[r::step]]
        assert seq == sorted(seq), (r, seq)
        assert seq[0] == 0
