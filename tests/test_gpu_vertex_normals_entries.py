"""mmx_vertex_normals / mmx_vertex_normals_backward on the GPU entry by entry: every entry of the normals, the sums and the
position gradient against the float64 reference under the per-entry rules of tests/vertex_normals_reference.py (forward_rule,
backward_rule; shown sound and with teeth on the CPU in tests/test_vertex_normals_reference.py), where
tests/test_gpu_vertex_normals.py takes the max-norm of an instance and allows 4 x the float32 reference's distance:

    sums            |x - x64| <= u |x64| + eps_v                                           eps_v = (n_v + 8) e A_v
    normals         |x_k - n_k| <= u |n_k| + (eps_k + |n_k| sum_j |n_j| eps_j) / M + 4 e |n_k|
    position_grad   |x - x64| <= u |x64| + (n_v + 16) e S_v                                x64 from the float32 sums the kernel is given

u = 2^-24, e = 2^-52; an exact zero where A, M or S is 0; positive zeros at a vertex of no triangle.  The meshes
(ref.ENTRY_MESHES) are the ones the max-norm suite cannot hold: every list length 0 .. 63 on the lanes of one wave and a group
without a row between live groups (ladder), valences 0 .. 200 on random triangles (soup_70, soup_300), faces folded shut to
10^-5 rad whose sums nearly cancel (books), centimetres away from the origin (cm), degenerate, exactly cancelling and live
triangles in one list (mixed), one vertex on one triangle (v1).  Then sums no forward gives (10^+-12, zeros, cotangents exactly
parallel to their sums), the exact laws of the design bit for bit (relabelling, scaling by powers of two, winding, removal of
degenerate triangles), NaN and inf at vertex 0 -- the vertex every padding record names -- and every write between guard blocks.

Measured on an MI355X (worst entry over the instances, error over what the rule allows, allowed 1;
profiles/vertex_normals_entry_bounds.json, written through MMX_PARITY_OUT by a run of this file alone):
    ladder                     normals 0.951   sums 0.945   position_grad 0.979
    soup_70                    normals 0.952   sums 0.980   position_grad 0.974
    soup_300                   normals 0.984   sums 0.981   position_grad 0.970
    books                      normals 0.982   sums 0.969   position_grad 0.978
    cm                         normals 0.979   sums 0.980   position_grad 0.996
    mixed                      normals 0.952   sums 0.980   position_grad 0.978
    v1                         normals 0       sums 0       position_grad 0 (exact zeros asked and given)
    ladder/arbitrary_sums                                   position_grad 0.963
    soup_70/arbitrary_sums                                  position_grad 0.940
    mixed/reversed_winding                                  position_grad 0.978
    books/reversed_winding                                  position_grad 0.978
Every entry holds its rule, and the figures are, to every digit shown, those of the float64 restatement of the kernels' order
on the CPU (tests/test_vertex_normals_reference.py): what is used of a bound is the one float32 rounding of the result, u |x64|,
and next to nothing of the e terms.  The same restatement with float32 accumulators is 70 to 1.1 x 10^6 times outside, with
float32 differences on cm 480 times.
"""
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import capi
from tests import vertex_normals_reference as ref

pytestmark = pytest.mark.gpu
_worst = {}
GUARD = 256  # floats of a guard block


@pytest.fixture(scope="module", autouse=True)
def _write_worst():
    """MMX_PARITY_OUT=<file>: the worst ratios of this run as JSON (how profiles/vertex_normals_entry_bounds.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _worst:
        unit = "worst entry over the instances: |x - x64| / (what the entry's rule allows), allowed = 1; the rules: tests/vertex_normals_reference.py"
        with open(out, "w") as f:
            json.dump(dict(unit=unit, cases=_worst), f, indent=1)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_gpu(mesh, pos, cot, sums=None):
    """normals and sums of the forward, position_grad from the forward's sums or from the ones given."""
    p = _cuda(pos)
    normals, fsums = mesh.vertex_normals(p, want_sums=True)
    grad = mesh.vertex_normals_backward(p, fsums if sums is None else _cuda(sums), _cuda(cot))
    return dict(normals=normals.cpu().numpy(), sums=fsums.cpu().numpy(), position_grad=grad.cpu().numpy())


def _assert_rules(name, pos, tri, cot, sums=None, got=None, keys=ref.KEYS):
    """The rules on every entry; returns the GPU's outputs."""
    V = pos.shape[1]
    if got is None:
        got = _run_gpu(capi.Mesh(tri, V), pos, cot, sums)
    rules = ref.forward_rule(pos, tri)
    rules["position_grad"] = ref.backward_rule(pos, tri, got["sums"] if sums is None else sums, cot)
    over = {}
    for key in keys:
        over[key] = ref.rule_ratios(got[key], rules[key])
        _worst[f"{name}/{key}"] = dict(ratio=float(over[key].max()), allowed=1.0)
        print(f"{name}/{key}: worst error / bound {over[key].max():.3g}")
    for key, r in over.items():
        at = np.unravel_index(np.argmax(r), r.shape)
        assert r.max() <= 1.0, (name, key, at, float(r.max()), got[key][at], rules[key]["want"][at], rules[key]["bound"][at])
    none = rules["entries"] == 0
    for key in keys:  # a vertex with no entry: positive zeros
        assert np.all(got[key][:, none] == 0.0) and not np.signbit(got[key][:, none]).any(), (name, key)
    return got


@pytest.mark.parametrize("name", list(ref.ENTRY_MESHES))
def test_every_entry_holds_its_rule(torch_cuda, name):
    pos, tri, cot = ref.entry_case(name)
    assert pos.shape[0] <= 3
    got = _assert_rules(name, pos, tri, cot)
    if name == "v1":
        for key in ref.KEYS:
            assert not _bits(got[key]).any(), key
    if name == "books":  # the nearly cancelling sums are there: A / |m| beyond 10^3 at the folds
        rule = ref.forward_rule(pos, tri)
        assert (np.linalg.norm(rule["A"], axis=-1) / np.linalg.norm(rule["sums"]["want"], axis=-1)).max() > 1e3


@pytest.mark.parametrize("name", ["ladder", "soup_70"])
def test_arbitrary_sums_entry_by_entry(torch_cuda, name):
    pos, tri, _ = ref.entry_case(name)
    sums, cot = ref.arbitrary_sums(pos.shape, 9)
    s = (sums.astype(np.float64) ** 2).sum(-1)
    assert (s == 0).sum() >= pos.shape[0] * pos.shape[1] // 7 and np.log10(s[s > 0].max() / s[s > 0].min()) > 40
    par = np.linalg.norm(np.cross(sums.astype(np.float64), cot.astype(np.float64)), axis=-1) == 0
    assert (par & (s > 0)).sum() >= s.size // 4
    got = _assert_rules(f"{name}/arbitrary_sums", pos, tri, cot, sums, keys=("position_grad",))
    # every h is zero where s = 0: with all sums zero the gradient is exact zeros
    zero = _run_gpu(capi.Mesh(tri, pos.shape[1]), pos, cot, np.zeros_like(sums))
    assert not zero["position_grad"].any() and np.isfinite(got["position_grad"]).all()


def _relabel(pos, tri, cot, perm):
    """Vertex v becomes perm[v]; the triangle list and the corner order stay."""
    new_pos, new_cot = np.empty_like(pos), np.empty_like(cot)
    new_pos[:, perm], new_cot[:, perm] = pos, cot
    return new_pos, perm[tri].astype(np.int32), new_cot


@pytest.mark.parametrize("name", ["ladder", "soup_300"])
def test_relabelling_the_vertices_permutes_the_outputs(torch_cuda, name):
    pos, tri, cot = ref.entry_case(name)
    V = pos.shape[1]
    base = _run_gpu(capi.Mesh(tri, V), pos, cot)
    for label, perm in (("reversal", np.arange(V)[::-1].copy()), ("random", np.random.default_rng(5).permutation(V)), ("plus_64", (np.arange(V) + 64) % V)):
        p2, t2, c2 = _relabel(pos, tri, cot, perm)
        got = _run_gpu(capi.Mesh(t2, V), p2, c2)
        for key in ref.KEYS:
            assert np.array_equal(_bits(got[key][:, perm]), _bits(base[key])), (label, key)


@pytest.mark.parametrize("name", ["soup_70", "books"])
def test_scaling_by_a_power_of_two(torch_cuda, name):
    pos, tri, cot = ref.entry_case(name)
    mesh = capi.Mesh(tri, pos.shape[1])
    base = _run_gpu(mesh, pos, cot)
    for k in (7, -10):
        f = np.float32(2.0**k)
        got = _run_gpu(mesh, pos * f, cot)
        assert np.array_equal(_bits(got["normals"]), _bits(base["normals"])), k
        assert np.array_equal(_bits(got["sums"]), _bits(base["sums"] * f * f)), k
        assert np.array_equal(_bits(got["position_grad"]), _bits(base["position_grad"] / f)), k


@pytest.mark.parametrize("name", ["mixed", "books"])
def test_reversed_winding_negates(torch_cuda, name):
    pos, tri, cot = ref.entry_case(name)
    base = _run_gpu(capi.Mesh(tri, pos.shape[1]), pos, cot)
    rev = np.ascontiguousarray(tri[:, [0, 2, 1]])
    got = _assert_rules(f"{name}/reversed_winding", pos, rev, cot, keys=("position_grad",))  # (the association of H changes)
    assert np.array_equal(got["sums"], -base["sums"]) and np.array_equal(got["normals"], -base["normals"])


def test_degenerate_triangles_add_nothing(torch_cuda):
    pos, tri, cot = ref.entry_case("mixed")
    V = pos.shape[1]
    dead = ref._is_degenerate(tri)
    assert dead.sum() == 24 and dead[0] and dead[-1]
    base = _run_gpu(capi.Mesh(tri, V), pos, cot)
    got = _run_gpu(capi.Mesh(np.ascontiguousarray(tri[~dead]), V), pos, cot)
    assert np.array_equal(got["normals"], base["normals"]) and np.array_equal(got["sums"], base["sums"])
    assert np.abs(base["sums"][:, :70]).max() > 0 and not base["sums"][:, 70:].any() and not base["normals"][:, 70:].any()


@pytest.mark.parametrize("name", ["ladder", "soup_70"])
def test_non_finite_values_at_vertex_0_stay_in_its_rings(torch_cuda, name):
    """Every padding record names vertex 0.  On ladder it has no triangle (its rings are itself: nothing may change at all);
    on soup_70 it has the longest list."""
    pos, tri, cot = ref.entry_case(name)
    V = pos.shape[1]
    mesh = capi.Mesh(tri, V)
    clean = _run_gpu(mesh, pos, cot)
    one, two = ref.rings(tri, V, 0)
    lone = name == "ladder"
    assert (one.sum() == 1) == lone and (two.sum() == 1) == lone and (lone or two.sum() > one.sum() > 10)

    def same_outside(got, key, ring, b):
        assert np.array_equal(_bits(got[key][b][~ring]), _bits(clean[key][b][~ring])), (key, b)
        assert np.array_equal(_bits(got[key][1 - b]), _bits(clean[key][1 - b])), (key, b)
        if lone:
            assert np.array_equal(_bits(got[key]), _bits(clean[key])), key

    for value in (np.nan, np.inf):
        bad = pos.copy()
        bad[1, 0, 1] = value
        got = _run_gpu(mesh, bad, cot)
        for key, ring in (("normals", one), ("sums", one), ("position_grad", two)):
            same_outside(got, key, ring, 1)
            if not lone:
                assert (~np.isfinite(got[key][1, ring])).any(axis=-1).all(), (key, value)
        for what in ("sums", "cot"):
            s, g = clean["sums"].copy(), cot.copy()
            (s if what == "sums" else g)[0, 0, 2] = value
            got = _run_gpu(mesh, pos, g, s)
            same_outside(got, "position_grad", one, 0)
            if not lone:
                assert np.isnan(got["position_grad"][0, one]).any(axis=-1).all(), (what, value)


NAN_PAYLOAD = 0x7FC0BEEF


@pytest.mark.parametrize("name", ["ladder", "v1"])
def test_every_entry_is_written_and_nothing_else(torch_cuda, name):
    """Each output is a view between two guard blocks of 256 floats of one allocation, prefilled with a NaN of a payload no
    arithmetic gives."""
    pos, tri, cot = ref.entry_case(name)
    B, V = pos.shape[:2]
    mesh = capi.Mesh(tri, V)
    plain = _run_gpu(mesh, pos, cot)
    n = B * V * 3
    full, inside = {}, {}
    for key in ref.KEYS:
        full[key] = torch.full((GUARD + n + GUARD,), -7.25, device="cuda")
        full[key][GUARD : GUARD + n].view(torch.int32).fill_(NAN_PAYLOAD)
        inside[key] = full[key][GUARD : GUARD + n].view(B, V, 3)
        assert inside[key].is_contiguous() and inside[key].data_ptr() == full[key].data_ptr() + 4 * GUARD
    p, g = _cuda(pos), _cuda(cot)
    L = capi.lib()
    capi._check(L.mmx_vertex_normals(mesh._h, B, capi._dev(p), capi._dev(inside["normals"]), capi._dev(inside["sums"]), capi._stream_ptr()))
    capi._check(L.mmx_vertex_normals_backward(mesh._h, B, capi._dev(p), capi._dev(inside["sums"]), capi._dev(g), capi._dev(inside["position_grad"]), capi._stream_ptr()))
    torch.cuda.synchronize()
    guard = _bits(np.full(GUARD, -7.25, np.float32))
    for key in ref.KEYS:
        a = full[key].cpu().numpy()
        assert np.array_equal(_bits(a[:GUARD]), guard) and np.array_equal(_bits(a[GUARD + n :]), guard), key  # nothing else
        assert not (_bits(a[GUARD : GUARD + n]) == NAN_PAYLOAD).any(), key  # every entry written
        assert np.array_equal(_bits(a[GUARD : GUARD + n]), _bits(plain[key]).reshape(-1)), key
