"""Static description of the reference's theta regressors: `Localizer` (model.py:152-184), `dense_homo` (:375-455) and
`flownetS_prehomo` (:897-959) with its twin `flownetS_variableWeight` (:962-1024).

Pure host logic like netspec.py, no torch / HIP: a layer table per graph, the spatial sizes for an H x W input, the variables'
names and shapes, synthetic variables with the graphs' initialisers, and the checkpoint key rule (netspec.ckpt_key /
strip_ckpt_keys with the builder's scope).

Confidence marks: ✔ = read off the reference's code, ⚠ = recalled from TensorFlow 1.x / TensorLayer 1.x (not in the reference's tree).

✔ every convolution is Conv2d(3x3, VALID, act=None) -> BatchNormLayer(act=lrelu 0.2, gamma_init=None); flownetS_prehomo and dense_homo
  put PadLayer([1,1],[1,1], "Symmetric") before each, Localizer pads nothing and its first convolution has stride 2.
✔ dense_homo's PadLayers all read `net_in` (model.py:385-402), so only conv2_3 / bn2_3 / pool2 reach the output; conv1_1..conv2_2 and
  their BatchNorms own variables that nothing reads (`DEAD`).
✔ DenseLayer(act=lrelu) -> BatchNormLayer(act=lrelu): the activation runs before and after the normalisation (model.py:953-956, 409-412).
✔ dense_homo's tail: tanh(x / 1000) * [0.3, 0.1, 170, 0.1, 0.3, 170, 0.01, 0.01] + [1, 0, 0, 0, 1, 0, 0, 0]; the concat with 1, the
  reshape to 3x3 and the slice [:, 0:8] (model.py:422-427) return those eight values unchanged.
⚠ variable names: Conv2d `<name>/W_conv2d` [3,3,cin,cout], `<name>/b_conv2d`; BatchNormLayer `<name>/beta`, `<name>/moving_mean`,
  `<name>/moving_variance` (no gamma with gamma_init=None), epsilon 1e-5; DenseLayer `<name>/W` [n_in, n_units], `<name>/b`.
⚠ FlattenLayer and ReshapeLayer([batch, -1]) flatten NHWC row-major: index (h * W + w) * C + c.
⚠ MaxPool2d((2,2),(2,2),'SAME') gives ceil(n / 2) and clips the window at an odd edge.
⚠ initialisers: tf.contrib.layers.variance_scaling_initializer() = N(0, 2 / fan_in) truncated; DenseLayer's default W_init is
  truncated_normal(stddev=0.1), b_init zeros.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import netspec

BN_EPS = netspec.BN_EPS
LRELU_SLOPE = 0.2                       # model.py:157, 380, 902
HOMO_SCALE = (0.3, 0.1, 170.0, 0.1, 0.3, 170.0, 0.01, 0.01)        # model.py:419
HOMO_SHIFT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)              # model.py:420


@dataclass(frozen=True)
class ConvStage:
    """Conv2d `name` (3x3, VALID) -> BatchNormLayer `bn` (lrelu 0.2), then a 2x2 SAME max pool when `pool`"""
    name: str
    bn: str
    cout: int
    stride: int = 1
    sym_pad: int = 1         # PadLayer "Symmetric" in front
    pool: bool = False


@dataclass(frozen=True)
class DenseStage:
    """DenseLayer `name` with `act` ('identity' | 'lrelu' | 'tanh' | 'tanh_affine'), then BatchNormLayer `bn` (lrelu 0.2) when named"""
    name: str
    units: Optional[int]     # None: the builder's out_param_dim
    act: str
    bn: Optional[str] = None


def _block(b: int, cout: int) -> Tuple[ConvStage, ...]:
    return tuple(ConvStage(f"conv{b}_{i}", f"bn{b}_{i}", cout, pool=(i == 3)) for i in (1, 2, 3))


@dataclass(frozen=True)
class Graph:
    name: str
    scope: str                                  # the builder's default variable scope
    convs: Tuple[ConvStage, ...]
    dense: Tuple[DenseStage, ...]
    dead: Tuple[ConvStage, ...] = ()            # layers whose variables exist and whose outputs nothing reads; all read the INPUT

    def sizes_for(self, H: int, W: int) -> "Sizes":
        h, w = int(H), int(W)
        conv: List[Tuple[int, int]] = []
        out: List[Tuple[int, int]] = []
        for st in self.convs:
            h = netspec.conv_out(h, 3, st.stride, st.sym_pad)
            w = netspec.conv_out(w, 3, st.stride, st.sym_pad)
            if H < 1 or W < 1 or h < 1 or w < 1:
                raise ValueError(f"input {H}x{W} too small for {self.name} (layer {st.name})")
            conv.append((h, w))
            if st.pool:
                h, w = (h + 1) // 2, (w + 1) // 2
            out.append((h, w))
        return Sizes(int(H), int(W), tuple(conv), tuple(out), h * w * self.convs[-1].cout)

    def dense_units(self, out_param_dim: Optional[int] = None) -> Tuple[int, ...]:
        units = []
        for d in self.dense:
            if d.units is None:
                if out_param_dim is None or int(out_param_dim) < 1:
                    raise ValueError(f"{self.name} needs out_param_dim >= 1")
                units.append(int(out_param_dim))
            else:
                units.append(d.units)
        return tuple(units)

    def weight_shapes(self, cin: int, H: int, W: int, out_param_dim: Optional[int] = None) -> Dict[str, Tuple[int, ...]]:
        """Short name -> shape of every variable of the graph for a [*, H, W, cin] input, the dead layers' included (a full
        reference checkpoint holds them)."""
        return self.shapes_from(cin, self.sizes_for(H, W).flat, self.dense_units(out_param_dim))

    def shapes_from(self, cin: int, flat: int, units: Tuple[int, ...]) -> Dict[str, Tuple[int, ...]]:
        """weight_shapes from the input channels, the first dense layer's K and the dense layers' units"""
        shp: Dict[str, Tuple[int, ...]] = {}

        def conv_vars(st, c):
            shp[f"{st.name}/W_conv2d"] = (3, 3, c, st.cout)
            shp[f"{st.name}/b_conv2d"] = (st.cout,)
            for v in ("beta", "moving_mean", "moving_variance"):
                shp[f"{st.bn}/{v}"] = (st.cout,)

        for st in self.dead:
            conv_vars(st, cin)
        c = cin
        for st in self.convs:
            conv_vars(st, c)
            c = st.cout
        n = flat
        for d, u in zip(self.dense, units):
            shp[f"{d.name}/W"] = (n, u)
            shp[f"{d.name}/b"] = (u,)
            if d.bn:
                for v in ("beta", "moving_mean", "moving_variance"):
                    shp[f"{d.bn}/{v}"] = (u,)
            n = u
        return shp

    def live_names(self, shapes) -> List[str]:
        """the variables of `shapes` that the output depends on"""
        dead = {st.name for st in self.dead} | {st.bn for st in self.dead}
        return [k for k in shapes if k.rsplit("/", 1)[0] not in dead]


@dataclass(frozen=True)
class Sizes:
    H: int
    W: int
    conv: Tuple[Tuple[int, int], ...]       # (h, w) each convolution writes
    out: Tuple[Tuple[int, int], ...]        # (h, w) each stage hands on (after its pool, where it has one)
    flat: int                               # K of the first dense layer: h * w * C of the last stage, NHWC order


LOCALIZER = Graph(
    "Localizer", "Localizer",
    convs=(ConvStage("d1/c1", "d1/b1", 32, stride=2, sym_pad=0), ConvStage("d2/c1", "d2/b1", 64, sym_pad=0),
           ConvStage("d3/c1", "d3/b1", 128, sym_pad=0), ConvStage("d4/c1", "d4/b1", 256, sym_pad=0),
           ConvStage("d5/c1", "d5/b1", 512, sym_pad=0)),
    dense=(DenseStage("df/dense1", 256, "identity", "df/b1"), DenseStage("df/dense2", None, "identity")))      # 'tanh' with is_tanh

PREHOMO = Graph(
    "flownetS_prehomo", "dense_homo",
    convs=_block(1, 64) + _block(2, 128) + _block(3, 256) + _block(4, 512),
    dense=(DenseStage("df/dense1", 256, "lrelu", "df/b1"), DenseStage("df/dense2", 128, "lrelu", "df/b2"),
           DenseStage("df/dense3", 8, "identity")))

DENSE_HOMO = Graph(
    "dense_homo", "dense_homo",
    convs=(ConvStage("conv2_3", "bn2_3", 128, pool=True),),
    dense=(DenseStage("df/dense1", 1000, "lrelu", "df/b1"), DenseStage("df/dense2", 1000, "lrelu", "df/b2"),
           DenseStage("df/dense3", 8, "tanh_affine")),
    dead=_block(1, 512) + _block(2, 512)[:2])

# flownetS_variableWeight (model.py:962-1024) repeats flownetS_prehomo line for line
GRAPHS: Dict[str, Graph] = {"Localizer": LOCALIZER, "flownetS_prehomo": PREHOMO, "flownetS_variableWeight": PREHOMO,
                            "dense_homo": DENSE_HOMO}


def graph(net: str) -> Graph:
    try:
        return GRAPHS[net]
    except KeyError:
        raise ValueError(f"unknown theta regressor {net!r} (one of {sorted(GRAPHS)})") from None


def ckpt_key(short: str, scope: str, outer: str = "main_net") -> str:
    """tensorlayer save_npz_dict key of a short variable name under the builder's scope (netspec.ckpt_key's rule)"""
    return netspec.ckpt_key(short, outer, scope)


def strip_ckpt_keys(d: dict, scope: str) -> dict:
    """short names from either short names or full `.../<scope>/<short>:0` keys (netspec.strip_ckpt_keys's rule)"""
    return netspec.strip_ckpt_keys(d, scope)


def synthetic_weights(net: str, seed: int = 1, cin: int = 27, H: int = 384, W: int = 512, out_param_dim: Optional[int] = None,
                      random_bn: bool = False, dense_std: float = 0.1) -> Dict[str, np.ndarray]:
    """Seeded variables with the graph's initialisers, short names: conv W ~ N(0, 2 / fan_in), dense W ~ N(0, dense_std^2) clipped
    at two sigma, biases 0, BatchNorm beta 0, mean 0, variance 1.  `random_bn=True` draws beta, mean ~ N(0, 0.1), variance ~ U(0.5, 1.5)
    and small biases, so that every term of the arithmetic matters (weights.synthetic_weights's convention)."""
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    for name, shp in graph(net).weight_shapes(cin, H, W, out_param_dim).items():
        leaf = name.rsplit("/", 1)[1]
        if leaf == "W_conv2d":
            w = rng.standard_normal(shp) * np.sqrt(2.0 / (shp[0] * shp[1] * shp[2]))
        elif leaf == "W":
            w = rng.standard_normal(shp, dtype=np.float32)          # float32 draws: Localizer's dense1 has 1.9e9 entries at 256 x 256
            np.clip(w, -2.0, 2.0, out=w)
            w *= np.float32(dense_std)
        elif leaf in ("b_conv2d", "b"):
            w = rng.standard_normal(shp) * 0.05 if random_bn else np.zeros(shp)
        elif leaf in ("beta", "moving_mean"):
            w = rng.standard_normal(shp) * 0.1 if random_bn else np.zeros(shp)
        elif leaf == "moving_variance":
            w = rng.uniform(0.5, 1.5, shp) if random_bn else np.ones(shp)
        else:  # pragma: no cover
            raise KeyError(name)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def validate(net: str, weights: Dict[str, np.ndarray], scope: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The graph's variables out of `weights` (short names or checkpoint keys), float32 and contiguous.  The input channels, the
    first dense layer's K and out_param_dim are read off the variables themselves; every other shape must follow from them.  The
    dead layers' variables are taken when present and not asked for."""
    g = graph(net)
    w = strip_ckpt_keys(weights, scope or g.scope)
    first, d1, dl = f"{g.convs[0].name}/W_conv2d", f"{g.dense[0].name}/W", f"{g.dense[-1].name}/W"
    for name in (first, d1, dl):
        if name not in w:
            raise KeyError(f"{g.name}: weights lack {name!r}")
        if np.asarray(w[name]).ndim != (4 if name == first else 2):
            raise ValueError(f"{g.name}: {name} has shape {np.asarray(w[name]).shape}")
    cin, K = int(np.asarray(w[first]).shape[2]), int(np.asarray(w[d1]).shape[0])
    units = g.dense_units(int(np.asarray(w[dl]).shape[1]))
    shapes = g.shapes_from(cin, K, units)
    live = set(g.live_names(shapes))
    out = {}
    for name, shp in shapes.items():
        if name not in w:
            if name in live:
                raise KeyError(f"{g.name}: missing variable {name!r}")
            continue
        a = np.ascontiguousarray(np.asarray(w[name]), dtype=np.float32)
        if tuple(a.shape) != tuple(shp):
            raise ValueError(f"{g.name}: {name} has shape {a.shape}, expected {shp}")
        out[name] = a
    return out
