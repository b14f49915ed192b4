"""CPU-side checks of the product package: the C ABI library loads and exports every
symbol include/gcm_hip.h declares, host logic (module wiring, state_dict keys, argument
validation) and the no-CPU-fallback rule.  No kernel is launched here."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from gcm import _hip
    header = open(os.path.join(ROOT, "include", "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", header))
    assert declared, "no prototypes parsed"
    lib = _hip.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in gcm_hip.h but not exported"
    assert declared == set(_hip.PROTOTYPES), declared ^ set(_hip.PROTOTYPES)
    assert lib.gcm_version() >= 100
    assert lib.gcm_status_string(-2).decode().startswith("shape not supported")


_SHAPES_HEADER = """
#ifndef T_H
#define T_H
#ifdef __cplusplus
extern "C" {
#endif
typedef void* gcm_stream_t; /* hipStream_t */
#define GCM_EBAD (-2) /* negative, parenthesised */
#define GCM_FOUR 4u
#define GCM_PLAIN 7
#define GCM_BYTES (160 * 1024)
typedef struct gcm_pair { int a, b; int32_t h[4]; const float* p; } gcm_pair;
int gcm_version(void);
size_t gcm_bytes(int B, int N);
const char* gcm_name(int code);
/* spread over several lines, comments between the parameters */
int gcm_many(const float* const* rows,   /* host array of device pointers */
             size_t* sizes,              // written
             long stride_a, long stride_b,
             int64_t M, float eps, const gcm_pair* pairs,
             gcm_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_shapes():
    """gcm/_abi.py on every declaration shape include/gcm_hip.h uses."""
    import ctypes as C
    from gcm import _abi
    text = _abi.strip_comments(_SHAPES_HEADER)
    assert _abi.prototypes(text) == {
        "gcm_version": (C.c_int, []),
        "gcm_bytes": (C.c_size_t, [C.c_int, C.c_int]),
        "gcm_name": (C.c_char_p, [C.c_int]),
        "gcm_many": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    }
    assert _abi.constants(text) == {"GCM_EBAD": -2, "GCM_FOUR": 4, "GCM_PLAIN": 7}     # the product is skipped
    assert _abi.struct_fields(text, "gcm_pair") == [("a", C.c_int), ("b", C.c_int), ("h", C.c_int32 * 4), ("p", C.c_void_p)]
    for bad in ("int gcm_odd(int a, unsigned b);", "double gcm_odd(int a);", "int gcm_odd(int a, long long b);"):
        with pytest.raises(TypeError, match="gcm_odd"):       # never guessed: raises, naming the function
            _abi.prototypes(text + bad)
    with pytest.raises(TypeError):
        _abi.prototypes(text + "int gcm_stray;")


def _top_level_commas(params):
    depth = n = 0
    for ch in params:
        depth += ch in "(["
        depth -= ch in ")]"
        n += ch == "," and depth == 0
    return n


def test_prototype_argument_counts_match_header():
    """Every bound prototype has as many argtypes as its declaration has top-level commas, plus one - counted on the
    header text, independently of the reader's type mapping."""
    from gcm import _hip
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gcm_hip.h")).read(), flags=re.S)
    decls = re.findall(r"\b(gcm_[a-z0-9_]+)\s*\((.*?)\)\s*;", header, flags=re.S)
    assert len(decls) == len(_hip.PROTOTYPES) == 150      # an ABI revision that adds or retires entry points updates this
    for name, params in decls:
        want = 0 if params.strip() == "void" else _top_level_commas(params) + 1
        assert len(_hip.PROTOTYPES[name][1]) == want, name


def test_constants_come_from_header():
    from gcm import _hip
    header = open(os.path.join(ROOT, "include", "gcm_hip.h")).read()
    assert f"#define GCM_ABI_VERSION {_hip.ABI_VERSION}\n" in header
    assert _hip.GCM_EUNSUPPORTED == -2 and _hip.FLAG_WINDOW == 128 and _hip.STEP_FOUR_WAVES == 256
    assert _hip.BPTT_MLP_BLOCKS == 256 and _hip.SPATIAL_MAX_COLS == 32
    assert _hip.DIR == {"forward": 1, "backward": 2, "both": 3}
    assert not hasattr(_hip, "SPATIAL_MAX_LDS")             # an expression, not a literal: left to C


def test_selector_desc_layout():
    """SelectorDesc against struct gcm_selector_desc: member names and order from the header text, and the size the C
    compiler gives it on LP64 with natural alignment:
      kind, n_hops 2 x 4 = 8 | hops[16] 64 -> 72 | direction, mode, max_distance 3 x 4 -> 84 | 4 padding -> 88 |
      dist_param 8 -> 96 | a0, a1, b0, b1, bidirectional 5 x 4 -> 116 | 4 padding -> 120 | cur_rows 8 -> 128 |
      n_cur_rows 4 -> 132 | 4 tail padding (alignment 8) -> 136."""
    import ctypes as C
    from gcm import _hip
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gcm_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gcm_selector_desc \{(.*?)\} gcm_selector_desc;", header, flags=re.S).group(1)
    names = [n for member in body.split(";") if member.strip()
             for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", member.strip())]
    assert [f[0] for f in _hip.SelectorDesc._fields_] == names and len(names) == 14
    assert C.sizeof(_hip.SelectorDesc) == 136
    assert (_hip.SelectorDesc.hops.offset, _hip.SelectorDesc.hops.size) == (8, 64)
    assert (_hip.SelectorDesc.dist_param.offset, _hip.SelectorDesc.cur_rows.offset, _hip.SelectorDesc.n_cur_rows.offset) == (88, 120, 128)


def test_argument_errors_without_gpu():
    """Host-side validation returns GCM_EINVAL before anything touches a device."""
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_graphconv_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_edge_dense(None, None, 1, 1, None) == -1
    assert lib.gcm_dense_graphconv_bwd_workspace_bytes(256, 128, 32, 32) > 0
    assert lib.gcm_edge_distance_workspace_bytes(0, 256, 128, 64) == (256 * 64 + 256) * 4   # rows + norms


def test_no_cpu_fallback():
    from gcm.gcm import DenseGCM
    from gcm import nn as G, _hip
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(4, 4), "x, adj -> x")])
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        DenseGCM(g, graph_size=4)(torch.zeros(2, 4), None)


def test_state_dict_keys_match_pyg_layout():
    from gcm import nn as G
    from oracle import pyg
    a = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(3, 5), "x, adj -> x"), torch.nn.Tanh(),
                                                (G.DenseGraphConv(5, 5), "x, adj -> x")])
    b = pyg.Sequential("x, adj, weights, B, N", [(pyg.DenseGraphConv(3, 5), "x, adj -> x"), torch.nn.Tanh(),
                                                  (pyg.DenseGraphConv(5, 5), "x, adj -> x")])
    assert list(a.state_dict()) == list(b.state_dict())
    assert "module_0.lin_rel.bias" in a.state_dict() and "module_0.lin_root.bias" not in a.state_dict()
    a.load_state_dict(b.state_dict())


def test_initial_hidden_state_and_asserts():
    from gcm.gcm import DenseGCM
    m = DenseGCM(torch.nn.Identity(), graph_size=6, edge_weights=True)
    nodes, adj, w, nn_ = m.get_initial_hidden_state(torch.zeros(3, 5))
    assert nodes.shape == (3, 6, 5) and adj.shape == (3, 6, 6) and w.shape == (3, 6, 6)
    assert nn_.dtype == torch.long and not nn_.any()
    m = DenseGCM(torch.nn.Identity(), graph_size=6)
    assert m.get_initial_hidden_state(torch.zeros(3, 5))[2].numel() == 0
    with pytest.raises(AssertionError):
        m(torch.zeros(3, 5, dtype=torch.float64), None)
    h = m.get_initial_hidden_state(torch.zeros(3, 5))
    with pytest.raises(AssertionError):
        m(torch.zeros(3, 5), (h[0], h[1], h[2], h[3].int()))


def test_selector_constructors():
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.distance import EuclideanEdge, CosineEdge, SpatialEdge
    with pytest.raises(AssertionError):
        TemporalBackedge([1], direction="sideways")
    e = EuclideanEdge(2.0, learned=True)
    assert e.max_distance == 1.0 and float(e.dist_param) == 2.0
    assert CosineEdge(0.5).max_distance == 0.5
    s = SpatialEdge(1.0, slice(0, 3))
    assert s._slices(8) == ((0, 3), (0, 3))


def test_util_straight_through_helpers():
    """util.Spardmax / Hardmax / diff_or (util.py:29-56, 456-465): host-side torch ops, checked
    against the oracle's per-row sparsemax restatement."""
    from gcm import util
    from oracle import dense as od
    torch.manual_seed(0)
    z = torch.randn(5, 9, requires_grad=True)
    p = util.sparsemax(z)
    for r in range(5):
        torch.testing.assert_close(p[r], od.sparsemax(z[r].detach()), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(util.sparsemax(z.t(), 0).t(), p)
    hard = util.Spardmax()(z)
    assert torch.equal(hard.detach(), (p > 0).float())
    hard.sum().backward()                      # straight through: the sparsemax gradient (rows sum to 1 -> 0)
    assert float(z.grad.abs().max()) < 1e-6
    hm = util.Hardmax(cutoff=0.2)(z.detach())
    assert torch.equal(hm, (torch.softmax(z.detach(), -1) > 0.2).float())
    a, b, c = (torch.tensor(v) for v in ([0., 1., 0., 1.], [0., 0., 1., 1.], [0., 0., 0., 1.]))
    assert torch.equal(util.diff_or([a, b, c]), torch.tensor([0., 1., 1., 1.]))
