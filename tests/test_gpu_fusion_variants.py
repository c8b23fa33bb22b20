"""-m gpu: every shipped instantiation of the fusion pack / unpack / cast kernels, bit for bit.

The product library dispatches the segment copy on the tile size (TIPS_COPY_TILE_BYTES 4096 / 8192 /
16384 -> U = 1 / 2 / 4) and the store policy (TIPS_COPY_STORE_POLICY -> POL = 0 / 1 / 2), the fused
cast on its tile (TIPS_CAST_TILE_BYTES -> U), the direction and the wire type, plus the sweep
variants TIPS_CAST_VARIANT 0-5 at U = 2 with an f16 wire; TIPS_COPY_ORDER (0 / 1 / 2) and
TIPS_PACK_STRIPE_KIB change which record slot a workgroup takes on the host (fusion.cc tile_order,
stripe_slots) and on the device (stripe_tile), which must stay one permutation. The other GPU tests
run the defaults only (U = 2, POL = 2, order 2, no stripes; the cast at U = 1, variant 8).

All runs are at one rank over fusion_cases' directed list (threshold 192 KiB: four buckets and one
tensor reduced where it lies), whose census of tile classes - the T/256-entry segment list, 3 and
more segments, two segments, a partial segment, a covering segment aligned and misaligned - is
asserted from the layout before every launch, in two placements (views aligned to 16 B with one
tensor a single element past; views packed one element apart). The reference is the input bytes
(random bytes: every bit pattern) or, for the cast, the oracle's casts of edge values; outputs,
inputs and the gaps between views are compared as integers, and a failure names the tensor, the byte
offset and the tile class. Every run must build a new pointer table (tips_fusion_stats): a cached
one is keyed on pointers and mode, not on the order, and would silently carry the previous order.

Which case reaches which kernel:
  test_copy_variants[tile, policy, order], U = tile / 4096, POL = policy, element sizes 2 / 4 / 8:
    in place, out of place (measure-pack on), flat with TIPS_PACK_MERGE=0  -> copy_segs_kernel<U, POL>
        over the slot tables' pack and unpack records and the flat table, one launch per bucket;
    out of place (measure-pack off)                                         -> copy_segs_kernel<U, POL>
        over the copy table, one launch over the whole space;
    flat with TIPS_PACK_MERGE=1                                             -> copy_segs_groups_kernel<U, POL>
        (three buckets in one launch, then one; no signals at one rank).
  test_cast_variants[tile, wire, placement], U = tile / 4096, WT = wire:
    every run                               -> cast_segs_kernel<U, 0, WT> and cast_segs_kernel<U, 1, WT>
        (variant 8: whole aligned tiles staged through LDS), and the range cast of the large tensor.
  test_striped_pack_child: TIPS_PACK_STRIPE_KIB=16 -> copy_segs_kernel<1 / 2 / 4, 2> with stripe > 0
        (in place, flat) and copy_segs_groups_kernel<1 / 2 / 4, 2> over stripe-ordered records (merged flat).
  test_cast_variant_child[v], v = 0-5 -> cast_segs_kernel<2, 0, f16, v> and cast_segs_kernel<2, 1, f16, v>
        (every tile through the quad path).
The last two knobs are read once per process, so each of those cases is one child process."""
import subprocess
import sys

import pytest

import fusion_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def release_input_bases():
    """fusion_cases keeps every input base allocated while this file runs (so that no case meets an
    earlier case's pointers, and with them its table); they go when the file is done."""
    yield
    fc._KEEP.clear()


@pytest.mark.parametrize("order", ["0", "1", "2"])
@pytest.mark.parametrize("policy", ["0", "1", "2"])
@pytest.mark.parametrize("tile", fc.TILES)
def test_copy_variants(gpu, monkeypatch, tile, policy, order):
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", str(tile))
    monkeypatch.setenv("TIPS_COPY_STORE_POLICY", policy)
    monkeypatch.setenv("TIPS_COPY_ORDER", order)
    seed = tile + 16 * int(policy) + 4 * int(order)
    for es in (2, 4, 8):
        for kind in ("aligned", "offset"):
            cen = fc.run_copy_routes(gpu, monkeypatch.setenv, es, kind, seed)
            assert cen.tile == tile


@pytest.mark.parametrize("kind", ["aligned", "offset"])
@pytest.mark.parametrize("wire", ["float16", "bfloat16"])
@pytest.mark.parametrize("tile", fc.TILES)
def test_cast_variants(gpu, monkeypatch, tile, wire, kind):
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_CAST_TILE_BYTES", str(tile))
    cen = fc.run_cast_routes(gpu, monkeypatch.setenv, wire, kind, tile)
    assert cen.tile == tile


def run_child(body, marker):
    """One fresh process (the knob under test is read once per process): it sets its environment,
    initialises the library, runs `body`, shuts down and prints `marker`."""
    from conftest import HERE, REPO
    code = ("import os, sys\nsys.path[:0] = [%r, %r]\n" % (REPO, HERE) + body +
            "\ntips_amd.shutdown()\nprint(%r)\n" % marker)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, timeout=240)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


def test_striped_pack_child():
    """TIPS_PACK_STRIPE_KIB=16: the pack launches deal 16 KiB stripes of record slots round-robin over
    the XCDs (stripe_tile) and tile_order places each XCD's boundary tiles by the same map
    (stripe_slots). The float32 list in place and flat (per-bucket and merged launches), at the three
    copy tiles; before launching, some bucket must hold more than 8 stripes' worth of tiles (else
    the launch falls back to contiguous eighths and nothing striped runs)."""
    run_child('''
os.environ.update(TIPS_PACK_STRIPE_KIB="16", TIPS_FUSION_THRESHOLD=str(%d))
import fusion_cases as fc
import tips_amd
tips_amd.init()
for tile in fc.TILES:
    os.environ["TIPS_COPY_TILE_BYTES"] = str(tile)
    for kind in ("aligned", "offset"):
        counts, names = fc.directed(4)
        pl = fc.Placement(counts, 4, kind, names["B"])
        ptrs = [(1 << 32) + 4 * s for s in pl.starts]
        cen = fc.census(counts, fc.F32, fc.SLOT, ptrs, ptrs)
        assert cen.tile == tile and max(cen.per_bucket) > 8 * (16384 // tile), (tile, cen.per_bucket)
        fc.run_copy_routes(tips_amd, os.environ.__setitem__, 4, kind, tile, routes=("inplace", "flat0", "flat1"))
''' % fc.THRESHOLD, "STRIPED_PACK_OK")


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_cast_variant_child(variant):
    """TIPS_CAST_VARIANT 0-5 (8 KiB cast tiles, f16 wire): plain or nt loads and the three store
    policies, every tile - whole aligned ones too - through the quad path."""
    run_child('''
os.environ.update(TIPS_CAST_VARIANT="%d", TIPS_CAST_TILE_BYTES="8192", TIPS_FUSION_THRESHOLD=str(%d))
import fusion_cases as fc
import tips_amd
tips_amd.init()
cen = fc.run_cast_routes(tips_amd, os.environ.__setitem__, "float16", "aligned", 100 + %d)
assert cen.tile == 8192
''' % (variant, fc.THRESHOLD, variant), "CAST_VARIANT_%d_OK" % variant)
