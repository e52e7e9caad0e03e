"""Tensor-level wrappers over the C ABI in include/coclr_hip.h.

Every function here takes device tensors (possibly channel-slice views of
wider NCDHW buffers), extracts raw pointers / strides and enqueues the HIP
kernel on torch's *current* stream.  Nothing is computed in Python or by
ATen, and there is no CPU path: host tensors are rejected.
"""
import ctypes as C
import os
import threading

import torch

from . import _lib
from . import plan as _plan
from ._lib import BnBwdCall, BnFwdCall, ConvCall, ConvDesc, PoolDesc


_HANDLE = None
_MAIN_THREAD = threading.get_ident()


def _desc(geom):
    """The launch descriptor of a cached geometry that THIS thread may fill in (strides, sample
    count): geometries are shared and cached, and the forward (caller's thread) and the backward
    (autograd's device thread) of different tensors may use one at the same time -- each side
    writes its own copy."""
    if threading.get_ident() == _MAIN_THREAD:
        return geom.desc
    d = geom.desc_bw
    if d is None:
        d = geom.desc_bw = type(geom.desc).from_buffer_copy(geom.desc)
    return d


def _L():
    """ctypes handle, resolved once (every wrapper below runs ~1500 times per step).  While THIS thread records a
    launch plan (coclr_amd/plan.py) the handle is the recorder's proxy: every entry point runs and is logged."""
    global _HANDLE
    if _HANDLE is None:
        _HANDLE = _lib.load()
    if _plan._ACTIVE is not None:
        rec = _plan.active()
        if rec is not None:
            return rec.proxy
    return _HANDLE


# Diagnostic: COCLR_HOST_DELAY_US=<n> burns n microseconds of host time per kernel launch.  If the step
# time does not move, the host is not on the critical path (tools/host_bound_probe.sh).
_HOST_DELAY = float(os.environ.get("COCLR_HOST_DELAY_US", "0")) * 1e-6


def _stream():
    if _HOST_DELAY:
        import time
        t = time.perf_counter() + _HOST_DELAY
        while time.perf_counter() < t:
            pass
    return torch.cuda.current_stream().cuda_stream


def _p(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.HipLibraryError(
            "coclr_amd: kernels need device tensors (got %s); there is no CPU fallback" % t.device)
    if t.dtype != dtype:
        raise TypeError("coclr_amd: expected %s tensor, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def _chk5(t, name):
    """NCDHW view whose (C,T,H,W) part is dense; returns the sample stride."""
    n, c, d, h, w = t.shape
    s = t.stride()
    if not (s[4] == 1 and s[3] == w and s[2] == h * w and s[1] == d * h * w) and t.numel() > 0:
        raise ValueError("coclr_amd: %s must be dense in (C,T,H,W); strides %s shape %s" %
                         (name, s, tuple(t.shape)))
    return s[0] if n > 1 else max(s[0], c * d * h * w)


WINOGRAD = os.environ.get("COCLR_WINOGRAD", "1") != "0"
WINOGRAD_HW = os.environ.get("COCLR_WINOGRAD_HW", "1") != "0"
# (3,1,1) layers through F(4,3) (algo = 2: six contractions per QUAD of output frames, 2x fewer MFMAs than the
# direct form) instead of F(2,3) (algo = 1: four per pair, 1.5x fewer); "0" keeps F(2,3)
WINOGRAD_T4 = os.environ.get("COCLR_WINO_T4", "1") != "0"
WINOGRAD_POLY7 = os.environ.get("COCLR_WINO_POLY7", "1") != "0"
WINOGRAD_PHASES = os.environ.get("COCLR_WINO_PHASES", "1") != "0"
_WINO_HW_MIN = int(os.environ.get("COCLR_WINO_HW_MIN", "16"))      # smallest map side that takes F(2x2,3x3)
_WINO_T4_MIN = int(os.environ.get("COCLR_WINO_T4_MIN", "16"))      # fewest frames that take F(4,3)


def winograd_ok(cin, k, s, p, d, lattice, odim=None, idim=None, algo=1):
    """Can this convolution run through the Winograd kernels (algo = 1)?  Stride-1 'same'
    convolutions of S3D's separable units (backbone/s3dg.py:39-42):
      * (3,1,1), pad (1,0,0): F(2,3) along T -- 4 channel contractions per pair of output frames
        instead of 6;
      * (1,3,3), pad (0,1,1), even H and W >= 4: F(2x2,3x3) -- 16 contractions per 2x2 output block
        instead of 36.
    Narrow layers stay direct (the kernels stage 8-16 channels at a time)."""
    k, p = tuple(k), tuple(p)
    if k == (7, 1, 1):
        # the stride-2 temporal stem conv in polyphase form (F(2,3) on the odd taps + F(2,4) on the even ones:
        # 9 contractions per pair of output frames instead of 14); forward only, even frame counts
        return (WINOGRAD and WINOGRAD_POLY7 and tuple(s) == (2, 1, 1) and p == (3, 0, 0) and
                tuple(d) == (1, 1, 1) and lattice is None and cin >= 16 and odim is not None and
                idim is not None and idim[0] == 2 * odim[0] and odim[0] >= 8)     # >= 4 output pairs per box
    if lattice is not None:
        # a destination lattice along T only, and only in the F(4,3) / F(2,4) kernels (algo = 2): the even / odd
        # phase of the strided temporal stem conv's data gradient (ConvGeom.dgrad_phases)
        ys, yo = tuple(lattice[0]), tuple(lattice[1])
        if not (algo == 2 and ys[1:] == (1, 1) and yo[1:] == (0, 0)):
            return False
    if not (WINOGRAD and tuple(s) == (1, 1, 1) and tuple(d) == (1, 1, 1)):
        return False
    if k == (4, 1, 1):
        return algo == 2 and p == (1, 0, 0) and cin >= 16 and odim is not None and idim is not None and \
            odim[0] == idim[0]
    if k == (3, 1, 1):
        return p == (1, 0, 0) and cin >= 16
    if k == (1, 3, 3):
        return (WINOGRAD_HW and p == (0, 1, 1) and cin >= 16 and odim is not None
                and odim[1] % 2 == 0 and odim[2] % 2 == 0 and odim[1] >= 4 and odim[2] >= 4)
    return False


def winograd_pays(cin, k, s, p, odim, idim=None):
    """Policy of conv_geom(): use Winograd where it is measurably faster.  The F(2x2,3x3) kernel
    holds one workgroup per CU; on 8x8 maps it only ties the direct kernel and on 4x4 maps it
    loses (profiles/r01_g_layers.txt), so the spatial form is kept for maps of 16x16 and up."""
    if not winograd_ok(cin, k, s, p, (1, 1, 1), None, odim, idim):
        return False
    if tuple(k) == (7, 1, 1):
        # measured at the benchmark shape only (32 -> 16 frames: 1.28 -> 1.09 ms, profiles/r06_poly7_ab.txt);
        # shorter clips keep the direct kernel
        return odim[0] >= 16
    return tuple(k) != (1, 3, 3) or (odim[1] >= _WINO_HW_MIN and odim[2] >= _WINO_HW_MIN)


def winograd_t4_pays(odim):
    """F(4,3) instead of F(2,3) for a (3,1,1) layer?  Measured per layer at B=32 (profiles/r06_wino_t4_layers.txt):
    16 frames (Conv_2c.conv2 0.754 -> 0.598 ms forward, Mixed_3c.b1.conv2 0.185 -> 0.145) yes; 8 frames (Mixed_4f
    0.080 -> 0.083) and 4 frames (Mixed_5c 0.050 -> 0.068: one quad per position, a third of the window is padding,
    three workgroups per CU instead of four) no."""
    return WINOGRAD_T4 and odim[0] >= _WINO_T4_MIN


class ConvGeom:
    """Geometry of one 3D convolution (python mirror of coclr_conv_desc)."""

    __slots__ = ("N", "Cin", "Cout", "idim", "odim", "k", "s", "p", "d", "lattice", "algo", "desc",
                 "desc_bw", "_cache")

    def __init__(self, N, Cin, Cout, idim, k, s, p, d=(1, 1, 1), odim=None, lattice=None, algo=0):
        self.N, self.Cin, self.Cout = int(N), int(Cin), int(Cout)
        self.idim = tuple(int(v) for v in idim)
        self.k, self.s, self.p, self.d = (tuple(int(v) for v in t) for t in (k, s, p, d))
        if odim is None:
            odim = tuple(((self.idim[i] - 1) * self.d[i] + 1 + 2 * self.p[i] - self.k[i]) //
                         self.s[i] + 1 for i in range(3))
        self.odim = tuple(int(v) for v in odim)
        if min(self.odim) <= 0:
            raise ValueError("coclr_amd: convolution output would be empty: in %s k %s s %s p %s" %
                             (self.idim, self.k, self.s, self.p))
        # lattice = (step, offset, full dims): output position o lands on element
        # o*step + offset of a tensor of extent `full dims` (one phase of a strided dgrad)
        self.lattice = lattice
        lat = (0,) * 9 if lattice is None else tuple(lattice[0]) + tuple(lattice[1]) + \
            tuple(lattice[2])
        # algo 1 = Winograd (see winograd_ok); the packed operand differs
        self.algo = int(algo)
        if self.algo not in (0, 1, 2):
            raise ValueError("coclr_amd: unknown convolution algorithm %d" % self.algo)
        if self.algo == 2 and self.k not in ((3, 1, 1), (4, 1, 1)):
            raise ValueError("coclr_amd: algorithm 2 is F(4,3) of a (3,1,1) stencil or F(2,4) of a (4,1,1) one")
        if self.algo >= 1 and not winograd_ok(self.Cin, self.k, self.s, self.p, self.d, lattice,
                                              self.odim, self.idim, self.algo):
            raise ValueError("coclr_amd: Winograd needs a (3,1,1) or (1,3,3) stride-1 'same' stencil, or the "
                             "(7,1,1) stride-2 pad-3 temporal stem conv on an even frame count")
        self.desc = ConvDesc(self.N, self.Cin, self.Cout, *self.idim, *self.odim, *self.k,
                             *self.s, *self.p, *self.d, 0, 0, *lat, 0, self.algo)
        self.desc_bw = None
        self._cache = {}

    @property
    def taps(self):
        return self.k[0] * self.k[1] * self.k[2]

    def dgrad(self):
        """Geometry of the data-gradient pass expressed as a forward call:
        stride-1 correlation of the zero-upsampled dY with the flipped stencil."""
        g = self._cache.get("dgrad")
        if g is None:
            pad = tuple(self.k[i] - 1 - self.p[i] for i in range(3))
            if min(pad) < 0:
                raise ValueError("coclr_amd: padding larger than kernel-1 is not supported")
            algo = self.algo if self.algo >= 1 and winograd_ok(self.Cout, self.k, (1, 1, 1), pad,
                                                               self.s, None, self.idim) else 0
            g = ConvGeom(self.N, self.Cout, self.Cin, self.odim, self.k, (1, 1, 1), pad,
                         d=self.s, odim=self.idim, algo=algo)
            self._cache["dgrad"] = g
        return g

    def dgrad_phases(self):
        """Data gradient of a conv strided along ONE axis whose stencil is 1 on the other
        two (S3D's temporal stem conv, backbone/s3dg.py:41), as `stride` dense stride-1
        correlations over dY, each writing one residue class of dX -- no multiply-by-zero
        work, unlike `dgrad()`.  Returns [(geom, tap_base, ntaps, tap_step)] or None when
        the geometry is not of that form."""
        g = self._cache.get("phases", False)
        if g is not False:
            return g
        out = None
        axes = [i for i in range(3) if self.s[i] > 1]
        if len(axes) == 1 and self.d == (1, 1, 1):
            ax = axes[0]
            others = [i for i in range(3) if i != ax]
            if all(self.k[i] == 1 and self.p[i] == 0 for i in others) and ax == 0:
                st, K, P = self.s[ax], self.k[ax], self.p[ax]
                out = []
                for phi in range(st):
                    k0 = (phi + P) % st
                    nk = (K - k0 + st - 1) // st
                    m_phi = (self.idim[ax] - phi + st - 1) // st
                    if nk not in (1, 3, 4) or m_phi <= 0:
                        out = None
                        break
                    c = (phi + P - k0) // st
                    kk, pp, od, ys, yo = [1, 1, 1], [0, 0, 0], list(self.idim), [1, 1, 1], [0, 0, 0]
                    kk[ax], pp[ax], od[ax], ys[ax], yo[ax] = nk, nk - 1 - c, m_phi, st, phi
                    # 3- and 4-tap phases of a long clip through F(4,3) / F(2,4) (algo = 2, lattice-aware kernels)
                    lat = (ys, yo, self.idim)
                    algo = 2 if (WINOGRAD_PHASES and winograd_t4_pays(od) and nk in (3, 4) and
                                 winograd_ok(self.Cout, tuple(kk), (1, 1, 1), tuple(pp), (1, 1, 1), lat,
                                             tuple(od), self.odim, 2)) else 0
                    geom = ConvGeom(self.N, self.Cout, self.Cin, self.odim, kk, (1, 1, 1), pp,
                                    odim=od, lattice=lat, algo=algo)
                    out.append((geom, k0, nk, st))
        self._cache["phases"] = out
        return out

    def ntiles(self):
        v = self._cache.get("ntiles")
        if v is None:
            out = C.c_int32(0)
            _lib.check(_L().coclr_conv3d_ntiles(C.byref(self.desc), C.byref(out)),
                       "conv3d_ntiles", self)
            v = self._cache["ntiles"] = out.value
        return v

    def bwd_sums_ok(self):
        """Can this problem's kernel form BatchNorm backward sums in its epilogue (conv_fwd_multi bwd_bn)?"""
        v = self._cache.get("bwd_sums_ok")
        if v is None:
            out = C.c_int32(0)
            _lib.check(_L().coclr_conv3d_bwd_sums_ok(C.byref(self.desc), C.byref(out)),
                       "conv3d_bwd_sums_ok", self)
            v = self._cache["bwd_sums_ok"] = bool(out.value)
        return v

    def wgrad_bn_ok(self):
        """Is there a weight-gradient kernel that applies the BatchNorm backward of the unit behind this
        convolution while it loads (conv_wgrad_bn)?"""
        v = self._cache.get("wgrad_bn_ok")
        if v is None:
            out = C.c_int32(0)
            _lib.check(_L().coclr_conv3d_wgrad_bn_ok(C.byref(self.desc), C.byref(out)),
                       "conv3d_wgrad_bn_ok", self)
            v = self._cache["wgrad_bn_ok"] = bool(out.value)
        return v

    def wgrad_workspace(self):
        v = self._cache.get("wgws")
        if v is None:
            out = C.c_int64(0)
            _lib.check(_L().coclr_conv3d_wgrad_workspace(C.byref(self.desc), C.byref(out)),
                       "conv3d_wgrad_workspace", self)
            v = self._cache["wgws"] = out.value
        return v

    def wgrad_plan(self, aligned=True, x_nstride=None, y_nstride=None):
        """What conv_wgrad would launch for this geometry, from the launcher's own planner (nothing is launched).
        aligned: x and dy both 16-byte aligned (the pointwise 16-byte-DMA kernels need it); x_nstride / y_nstride:
        the operands' sample strides (default: dense tensors)."""
        d = ConvDesc.from_buffer_copy(self.desc)
        d.x_nstride = x_nstride or self.Cin * self.idim[0] * self.idim[1] * self.idim[2]
        d.y_nstride = y_nstride or self.Cout * self.odim[0] * self.odim[1] * self.odim[2]
        out = (C.c_int32 * 16)()
        _lib.check(_L().coclr_conv3d_wgrad_plan(C.byref(d), int(bool(aligned)), out), "conv3d_wgrad_plan", self)
        family = ("gen1", "wave", "stem", "pwdma")[out[0]]
        return dict(family=family, id=out[1], pch=out[2], bj=out[3], split=out[4], slices=out[5], ct=out[6],
                    mt=out[7], lTW=out[8], lTH=out[9], lTT=out[10], lTN=out[11], ntiles=out[12],
                    tile_order=bool(out[13]), bn=bool(out[14]), rebox=bool(out[15]))

    _FWD_FAMILIES = ("igemm", "wino_t", "wino_tf", "wino_hw", "wino_hw8", "stem")
    _FWD_FIELDS = ("variant", "family", "form", "KT", "KH", "KW", "CC", "BM", "BN", "PCH", "OCC", "XV4", "XG",
                   "X16", "INAFF", "lattice", "pairable", "lTW", "lTH", "lTT", "lTN", "WT", "WH", "WW", "plane",
                   "ntiles", "mtiles", "nchunks", "planeS", "lds", "grid", "threads", "slot_filled", "nboxes",
                   "nbw", "nbh", "nbt", "nbn", "bwd_sums_ok")

    def fwd_plan(self, x_aligned=True, y_aligned=True, n_index=False, in_affine=False, slot=False,
                 bwd_sums=False, x_nstride=None, y_nstride=None, Nx=None):
        """What conv_fwd / conv_fwd_multi would launch for this geometry, from the launcher's own planner and
        kernel selection (nothing is launched): a dict of the fields of coclr_conv3d_fwd_plan, `family` by name,
        the flags as bools.  x_aligned: x is 16-byte aligned; y_aligned: y is 8-byte aligned; x_nstride /
        y_nstride / Nx: the operands' sample strides and the samples behind an n_index (default: dense tensors).
        A combination the launch refuses raises HipLibraryError exactly as the launch would."""
        d = ConvDesc.from_buffer_copy(self.desc)
        d.x_nstride = x_nstride or self.Cin * self.idim[0] * self.idim[1] * self.idim[2]
        if y_nstride is None:
            full = self.lattice[2] if self.lattice is not None else self.odim
            y_nstride = self.Cout * full[0] * full[1] * full[2]
        d.y_nstride = y_nstride
        d.Nx = Nx or self.N
        flags = (1 * bool(x_aligned) | 2 * bool(y_aligned) | 4 * bool(n_index) | 8 * bool(in_affine) |
                 16 * bool(slot) | 32 * bool(bwd_sums))
        out = (C.c_int32 * 40)()
        _lib.check(_L().coclr_conv3d_fwd_plan(C.byref(d), flags, out), "conv3d_fwd_plan", self)
        r = dict(zip(self._FWD_FIELDS, out))
        r["family"] = self._FWD_FAMILIES[r["family"]]
        for k in ("XV4", "XG", "X16", "INAFF", "lattice", "pairable", "slot_filled", "bwd_sums_ok"):
            r[k] = bool(r[k])
        return r

    def __repr__(self):
        return "ConvGeom(N=%d, %d->%d, in=%s, out=%s, k=%s, s=%s, p=%s, d=%s)" % (
            self.N, self.Cin, self.Cout, self.idim, self.odim, self.k, self.s, self.p, self.d)


_GEOMS = {}


def conv_geom(N, Cin, Cout, idim, k, s, p):
    """Shared, cached ConvGeom (its ntiles / dgrad / phase plans are computed once): the engine
    asks for the same ~80 geometries every step.  Picks the algorithm (direct / Winograd)."""
    key = (N, Cin, Cout, tuple(idim), tuple(k), tuple(s), tuple(p))
    g = _GEOMS.get(key)
    if g is None:
        if len(_GEOMS) > 8192:
            _GEOMS.clear()
        g = ConvGeom(N, Cin, Cout, idim, k, s, p)
        if winograd_pays(Cin, k, s, p, g.odim, g.idim):
            g = ConvGeom(N, Cin, Cout, idim, k, s, p,
                         algo=2 if (tuple(k) == (3, 1, 1) and winograd_t4_pays(g.odim)) else 1)
        _GEOMS[key] = g
    return g


def pool_geom(N, Cc, idim, k, s, p):
    key = ("pool", N, Cc, tuple(idim), tuple(k), tuple(s), tuple(p))
    g = _GEOMS.get(key)
    if g is None:
        g = _GEOMS[key] = PoolGeom(N, Cc, idim, k, s, p)
    return g


class PoolGeom:
    __slots__ = ("N", "C", "idim", "odim", "k", "s", "p", "desc", "desc_bw", "_pooled_fits")

    def __init__(self, N, Cc, idim, k, s, p):
        self.N, self.C = int(N), int(Cc)
        self.idim = tuple(int(v) for v in idim)
        self.k, self.s, self.p = (tuple(int(v) for v in t) for t in (k, s, p))
        self.odim = tuple((self.idim[i] + 2 * self.p[i] - self.k[i]) // self.s[i] + 1
                          for i in range(3))
        if min(self.odim) <= 0:
            raise ValueError("coclr_amd: pooling output would be empty")
        self.desc = PoolDesc(self.N, self.C, *self.idim, *self.odim, *self.k, *self.s, *self.p, 0, 0)
        self.desc_bw = None
        self._pooled_fits = None

    _FWD_FAMILIES = ("generic", "sep333", "tiled")
    _FWD_TILED = ((1, 3, 3, 1, 2, 2, 2), (3, 3, 3, 1, 1, 1, 4), (3, 3, 3, 2, 2, 2, 2), (2, 2, 2, 2, 2, 2, 2))
    _BWD_FAMILIES = ("generic", "gather333", "classes")

    def plan(self, with_indices=True, x_nstride=None, y_nstride=None, dy_nstride=None, dx_nstride=None):
        """What maxpool_fwd, maxpool_bwd and bn_act_backward_pooled would launch for this geometry, from the
        launchers' own plan structs (nothing is launched): dict(fwd=..., bwd=..., pooled=..., nt=...).  The strides
        are the operands' sample strides (default: dense tensors); the pooled BatchNorm backward is planned with
        y at x_nstride and its dy at dx_nstride.  The `vec` flags are what the launchers hand the kernels.  `template` is TT for the separable forward, the (KT, KH, KW, ST, SH, SW, WPT) row
        for the tiled forward and (PT, PH, PW, KQ) for the colour-class forms, (0, 0, 0, 0) the generic form."""
        d = PoolDesc.from_buffer_copy(self.desc)
        si = self.idim[0] * self.idim[1] * self.idim[2]
        so = self.odim[0] * self.odim[1] * self.odim[2]
        d.x_nstride = x_nstride or self.C * si
        d.y_nstride = y_nstride or self.C * so
        out = (C.c_int32 * 32)()
        _lib.check(_L().coclr_pool_plan(C.byref(d), int(bool(with_indices)), dy_nstride or 0, dx_nstride or 0,
                                        out), "pool_plan", self)
        fam = self._FWD_FAMILIES[out[0]]
        fwd = dict(family=fam, G=out[2], grid=(out[3], out[4]), tfold=out[5], vec=bool(out[6]), lds=out[7],
                   template=None if fam == "generic" else out[1] if fam == "sep333" else self._FWD_TILED[out[1]])
        bfam = self._BWD_FAMILIES[out[8]]
        bwd = dict(family=bfam, template=tuple(out[9:13]) if bfam == "classes" else None, G=out[13], kq=out[14],
                   grid=(out[15], out[16]), tfold=out[17], vec=bool(out[18]), lds=out[19])
        pooled = dict(fits=bool(out[20]), G=out[21], template=tuple(out[22:26]) if out[20] else None, kq=out[26],
                      blocks=out[27], tfold=out[28], vec=bool(out[29]), lds=out[30])
        return dict(fwd=fwd, bwd=bwd, pooled=pooled, nt=bool(out[31]))

    def __repr__(self):
        return "PoolGeom(N=%d, C=%d, in=%s, k=%s, s=%s, p=%s)" % (self.N, self.C, self.idim, self.k, self.s, self.p)


# ---- convolution ---------------------------------------------------------------

_PACKED = {}


def conv_packed_size(cin, cout, taps, transpose):
    key = (cin, cout, taps, bool(transpose))
    v = _PACKED.get(key)
    if v is not None:
        return v
    v = _PACKED[key] = _conv_packed_size(cin, cout, taps, transpose)
    return v


def _conv_packed_size(cin, cout, taps, transpose):
    out = C.c_int64(0)
    _lib.check(_L().coclr_conv_packed_size(cin, cout, taps, int(transpose), C.byref(out)),
               "conv_packed_size")
    return out.value


def conv_pack_weights(w, packed, cout, cin, taps, co_stride, ci_stride, tap_base, transpose,
                      tap_step=1, row0=0, rows_total=0, col0=0, cols_total=0):
    _lib.check(_L().coclr_conv_pack_weights(
        _p(w), _p(packed), cout, cin, taps, co_stride, ci_stride, tap_base, tap_step,
        int(transpose), row0, rows_total, col0, cols_total, _stream()), "conv_pack_weights")


def conv_pack_describe(w, packed, cout, cin, taps, co_stride, ci_stride, tap_base, transpose,
                       tap_step=1, row0=0, rows_total=0, col0=0, cols_total=0):
    """One row of a batch-pack table (16 int64) and the number of 1024-element blocks it takes;
    same arguments as conv_pack_weights."""
    entry = (C.c_int64 * 16)()
    nb = C.c_int32()
    _lib.check(_L().coclr_conv_pack_describe(
        _p(w), _p(packed), cout, cin, taps, co_stride, ci_stride, tap_base, tap_step,
        int(transpose), row0, rows_total, col0, cols_total, entry, C.byref(nb)), "conv_pack_describe")
    return list(entry), nb.value


def conv_pack_batch(table, blockmap, requests=None):
    """Launch every re-layout of a table built from conv_pack_describe rows.  `requests` (the
    argument tuples the rows were made from) is unused here; the CPU test double replays them."""
    _lib.check(_L().coclr_conv_pack_batch(_p(table, torch.int64), _p(blockmap, torch.int32),
                                          blockmap.shape[0], _stream()), "conv_pack_batch")


def conv_fwd(geom, x, w_packed, y, stats=None, bias=None, ep_scale=None, ep_shift=None,
             n_index=None, relu=False, accumulate=False):
    d = _desc(geom)
    d.x_nstride = _chk5(x, "x")
    d.y_nstride = _chk5(y, "y")
    d.Nx = x.shape[0]
    _lib.check(_L().coclr_conv3d_fwd(
        C.byref(d), _p(x), _p(w_packed), _p(y), _p(stats), _p(bias), _p(ep_scale), _p(ep_shift),
        _p(n_index, torch.int64), int(relu), int(accumulate), _stream()), "conv3d_fwd", geom)


def conv_fwd_multi(calls):
    """Independent convolutions in one call (consecutive pairs of the same kernel variant in one launch).
    calls: [dict(geom, x, w, y, stats=None, n_index=None, accumulate=False, bwd_bn=None)]; every problem keeps
    the plan it has alone (statistics: geom.ntiles() slots per channel).  bwd_bn = (y, scale, shift, mean,
    invstd, relu) of a BatchNorm unit: the problem is the data gradient that writes that unit's dz and `stats`
    receives the unit's backward sums (include/coclr_hip.h, coclr_conv_call)."""
    n = len(calls)
    arr = (ConvCall * n)()
    descs = []
    for i, c in enumerate(calls):
        geom, x, y = c["geom"], c["x"], c["y"]
        # every problem gets its OWN descriptor copy: two problems may share one cached geometry
        d = type(geom.desc).from_buffer_copy(_desc(geom))
        d.x_nstride = _chk5(x, "x")
        d.y_nstride = _chk5(y, "y")
        d.Nx = x.shape[0]
        descs.append(d)
        a = arr[i]
        a.d = C.pointer(d)
        a.x, a.w_packed, a.y = _p(x), _p(c["w"]), _p(y)
        a.stats = _p(c.get("stats"))
        a.bias = a.ep_scale = a.ep_shift = None
        a.n_index = _p(c.get("n_index"), torch.int64)
        a.relu = 0
        a.accumulate = int(bool(c.get("accumulate", False)))
        ia = c.get("in_affine")
        if ia is not None:
            # (scale, shift, relu) of the BatchNorm unit whose raw output x is: applied while the kernel reads
            a.in_scale, a.in_shift, a.in_relu = _p(ia[0]), _p(ia[1]), int(bool(ia[2]))
        bb = c.get("bwd_bn")
        if bb is not None:
            # (y, scale, shift, mean, invstd, relu) of the BatchNorm unit whose dz this data gradient writes
            by = bb[0]
            if by.shape != y.shape or _chk5(by, "bwd_y") != d.y_nstride or not y.is_contiguous():
                raise ValueError("coclr_amd: bwd_bn's conv output must be laid out like the destination")
            a.bwd_y, a.bwd_scale, a.bwd_shift = _p(by), _p(bb[1]), _p(bb[2])
            a.bwd_mean, a.bwd_invstd, a.bwd_relu = _p(bb[3]), _p(bb[4]), int(bool(bb[5]))
    _lib.check(_L().coclr_conv3d_fwd_multi(arr, n, _stream()), "conv3d_fwd_multi",
               [c["geom"] for c in calls])


def conv_wgrad(geom, x, dy, dw, workspace, co_stride, ci_stride, tap_base, accumulate=False):
    """dw: the gradient tensor, or a list of up to four tensors that take consecutive blocks of
    output-channel rows (dw[i].shape[0] rows each, summing to geom.Cout)."""
    d = _desc(geom)
    d.x_nstride = _chk5(x, "x")
    d.y_nstride = _chk5(dy, "dy")
    if isinstance(dw, (list, tuple)):
        n = len(dw)
        ptrs = (C.c_void_p * n)(*[_p(t) for t in dw])
        ends, tot = [], 0
        for t in dw:
            tot += t.shape[0]
            ends.append(tot)
        _lib.check(_L().coclr_conv3d_wgrad_multi(
            C.byref(d), _p(x), _p(dy), ptrs, (C.c_int32 * n)(*ends), n, _p(workspace), co_stride,
            ci_stride, tap_base, int(accumulate), _stream()), "conv3d_wgrad_multi", geom)
        return
    _lib.check(_L().coclr_conv3d_wgrad(
        C.byref(d), _p(x), _p(dy), _p(dw), _p(workspace), co_stride, ci_stride, tap_base,
        int(accumulate), _stream()), "conv3d_wgrad", geom)


def conv_wgrad_bn(geom, x, dz, y, coef, relu, dw, workspace, co_stride, ci_stride, tap_base=0,
                  accumulate=False):
    """conv_wgrad over dy = BatchNorm(+ReLU) backward of (dz, y) formed on the fly (coef from
    bn_act_backward_coeffs); geom.wgrad_bn_ok() geometries only."""
    d = _desc(geom)
    d.x_nstride = _chk5(x, "x")
    d.y_nstride = _chk5(dz, "dz")
    _lib.check(_L().coclr_conv3d_wgrad_bn(
        C.byref(d), _p(x), _p(dz), _p(y), _chk5(y, "y"), _p(coef), int(relu), _p(dw), _p(workspace),
        co_stride, ci_stride, tap_base, int(accumulate), _stream()), "conv3d_wgrad_bn", geom)


# ---- batch norm ------------------------------------------------------------------

def bn_finalize(stats, C_, ntiles, count, gamma, beta, running_mean, running_var, nbt, momentum,
                eps, mean, invstd, scale, shift, c0=0, c_total=None):
    """stats: [2][c_total][ntiles] partial sums of a convolution with c_total output channels;
    this call finalises channels [c0, c0+C_)."""
    c_total = C_ if c_total is None else c_total
    base = _p(stats)
    _lib.check(_L().coclr_bn_finalize(
        base + 4 * c0 * ntiles, base + 4 * (c_total + c0) * ntiles, C_, ntiles, float(count),
        _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(nbt, torch.int64), momentum, eps,
        _p(mean), _p(invstd), _p(scale), _p(shift), _stream()), "bn_finalize")


def bn_finalize_apply(stats, C_, ntiles, count, gamma, beta, running_mean, running_var, nbt,
                      momentum, eps, mean, invstd, scale, shift, y, z, relu, c0=0, c_total=None):
    """bn_finalize + bn_act_apply (no residual) in one call; a single launch for small layers.
    y: the [N][C_][S] channel range (a view) the statistics belong to."""
    c_total = C_ if c_total is None else c_total
    base = _p(stats)
    N, _, T, H, W = y.shape
    _lib.check(_L().coclr_bn_finalize_apply(
        base + 4 * c0 * ntiles, base + 4 * (c_total + c0) * ntiles, C_, ntiles, float(count),
        _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(nbt, torch.int64), momentum, eps,
        _p(mean), _p(invstd), _p(scale), _p(shift), _p(y), _p(z), N, T * H * W, _chk5(y, "y"),
        _chk5(z, "z"), int(relu), _stream()), "bn_finalize_apply")


def bn_finalize_apply_multi(units):
    """bn_finalize_apply for several units in one call (one launch for runs of small units).
    units: [dict(stats, C, ntiles, count, bn=(gamma, beta, running_mean, running_var, nbt, momentum, eps),
    small=(mean, invstd, scale, shift), y, z, relu, c0=0, c_total=None)]."""
    n = len(units)
    arr = (BnFwdCall * n)()
    for a, u in zip(arr, units):
        C_, ntiles = u["C"], u["ntiles"]
        c0 = u.get("c0", 0)
        c_total = u.get("c_total") or C_
        base = _p(u["stats"])
        gamma, beta, rm, rv, nbt, momentum, eps = u["bn"]
        mean, invstd, scale, shift = u["small"]
        y, z = u["y"], u["z"]
        N, _, T, H, W = y.shape
        a.sum = base + 4 * c0 * ntiles
        a.sumsq = base + 4 * (c_total + c0) * ntiles
        a.gamma, a.beta, a.running_mean, a.running_var = _p(gamma), _p(beta), _p(rm), _p(rv)
        a.num_batches_tracked = _p(nbt, torch.int64)
        a.mean, a.invstd, a.scale, a.shift = _p(mean), _p(invstd), _p(scale), _p(shift)
        a.y, a.z = _p(y), _p(z)
        a.count = float(u["count"])
        a.S = T * H * W
        a.y_nstride, a.z_nstride = _chk5(y, "y"), _chk5(z, "z")
        a.C, a.ntiles, a.N, a.relu = C_, ntiles, N, int(u["relu"])
        a.momentum, a.eps = momentum, eps
    _lib.check(_L().coclr_bn_finalize_apply_multi(arr, n, _stream()), "bn_finalize_apply_multi")


def bn_act_backward_multi(units):
    """bn_act_backward (no residual) for several units in one call.
    units: [dict(dz, y, scale, shift, mean, invstd, sums, dy, dgamma, dbeta, relu, training, partials=None)];
    partials = [(stats, ntiles)] formed by the data gradient that wrote dz (conv_fwd_multi bwd_bn)."""
    n = len(units)
    arr = (BnBwdCall * n)()
    for a, u in zip(arr, units):
        y = u["y"]
        N, C_, T, H, W = y.shape
        if u["sums"].numel() < 2 * C_ * N:
            raise ValueError("coclr_amd: bn_act_backward workspace too small")
        a.dz, a.y, a.scale, a.shift = _p(u["dz"]), _p(y), _p(u["scale"]), _p(u["shift"])
        a.mean, a.invstd = _p(u["mean"]), _p(u["invstd"])
        a.sums_ws = _p(u["sums"], torch.float64)
        a.dy, a.dgamma, a.dbeta = _p(u["dy"]), _p(u["dgamma"]), _p(u["dbeta"])
        a.S = T * H * W
        a.dz_nstride, a.y_nstride, a.dy_nstride = _chk5(u["dz"], "dz"), _chk5(y, "y"), _chk5(u["dy"], "dy")
        a.N, a.C, a.relu, a.training = N, C_, int(u["relu"]), int(u["training"])
        parts = u.get("partials")
        if parts:
            # [(stats, ntiles)] left by the data gradient(s) that wrote dz: no reduction pass
            if len(parts) > 2:
                raise ValueError("coclr_amd: at most two partial-sum arrays per BatchNorm backward")
            for i, (st, nt) in enumerate(parts):
                if st.numel() != 2 * C_ * nt:
                    raise ValueError("coclr_amd: partial sums do not match the unit's channels")
                a.part[i] = _p(st)
                a.part_ntiles[i] = nt
    _lib.check(_L().coclr_bn_act_backward_multi(arr, n, _stream()), "bn_act_backward_multi")


SMALL_CHANNEL = 32768      # N*S per channel up to which the one-launch BatchNorm forms are used


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, C_, mean, invstd, scale, shift):
    _lib.check(_L().coclr_bn_eval_affine(
        _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, C_, _p(mean), _p(invstd),
        _p(scale), _p(shift), _stream()), "bn_eval_affine")


def bn_act_apply(y, scale, shift, residual, z, relu):
    N, C_, T, H, W = y.shape
    S = T * H * W
    _lib.check(_L().coclr_bn_act_apply(
        _p(y), _p(scale), _p(shift), _p(residual), _p(z), N, C_, S, _chk5(y, "y"), _chk5(z, "z"),
        _chk5(residual, "residual") if residual is not None else 0, int(relu), _stream()),
        "bn_act_apply")


def bn_plan(N, C_, S, y_nstride=None, z_nstride=None, dz_nstride=None, dy_nstride=None, dres_nstride=None,
            has_z=False, has_dres=False, has_partials=False):
    """The routes of one BatchNorm unit, from the launchers' own route struct (nothing is launched):
    dict(fwd=..., bwd=...), each with one_wg (one workgroup per channel), vec, nt and the streaming pass's
    plane grid; bwd also has `groups` (sample groups of the reduce pass, 0: none) and `partials`.  Strides
    default to dense tensors."""
    dense = C_ * S
    out = (C.c_int32 * 16)()
    _lib.check(_L().coclr_bn_plan(N, C_, S, y_nstride or dense, z_nstride or dense, dz_nstride or dense,
                                  dy_nstride or dense, dres_nstride or dense, int(bool(has_z)),
                                  int(bool(has_dres)), int(bool(has_partials)), out), "bn_plan")
    return dict(fwd=dict(one_wg=bool(out[0]), vec=bool(out[1]), nt=bool(out[2]), grid=(out[3], out[4])),
                bwd=dict(one_wg=bool(out[5]), vec=bool(out[6]), nt=bool(out[7]), groups=out[8],
                         grid=(out[9], out[10]), partials=bool(out[11])))


def bn_multi_plan(units, backward=False):
    """How bn_finalize_apply_multi (or, with backward, bn_act_backward_multi) would cut these units into launches,
    from the launchers' own run-cutting function (nothing is launched): a list of run lengths (>= 2: one fused
    launch, 1: the unit goes alone).  units: [dict(N, C, S, y_nstride, z_nstride)] or, backward,
    [dict(N, C, S, dz_nstride, y_nstride, dy_nstride, partials=False)]; strides default to dense."""
    n = len(units)
    arr = ((BnBwdCall if backward else BnFwdCall) * n)()
    for a, u in zip(arr, units):
        dense = u["C"] * u["S"]
        a.N, a.C, a.S = u["N"], u["C"], u["S"]
        a.y = 16                      # operands only have to be non-null: nothing is dereferenced
        a.y_nstride = u.get("y_nstride") or dense
        if backward:
            a.dz = a.dy = 16
            a.dz_nstride, a.dy_nstride = u.get("dz_nstride") or dense, u.get("dy_nstride") or dense
            if u.get("partials"):
                a.part[0] = 16
                a.part_ntiles[0] = 1
        else:
            a.z, a.ntiles = 16, 1
            a.z_nstride = u.get("z_nstride") or dense
    out = (C.c_int32 * (n + 1))()
    _lib.check(_L().coclr_bn_multi_plan(None if backward else arr, arr if backward else None, n, out),
               "bn_multi_plan")
    return [v for v in out[:n] if v]


def bn_backward_workspace(N, C_):
    """float64 elements of the partial-sum workspace of bn_act_backward."""
    return 2 * C_ * N


def bn_act_backward(dz, y, z, scale, shift, mean, invstd, sums_ws, dy, dres, dgamma, dbeta, relu,
                    training, dres_accumulate=False):
    N, C_, T, H, W = y.shape
    S = T * H * W
    if sums_ws.numel() < 2 * C_ * N:
        raise ValueError("coclr_amd: bn_act_backward workspace too small")
    _lib.check(_L().coclr_bn_act_backward(
        _p(dz), _p(y), _p(z), _p(scale), _p(shift), _p(mean), _p(invstd),
        _p(sums_ws, torch.float64), _p(dy), _p(dres), _p(dgamma), _p(dbeta), N, C_, S,
        _chk5(dz, "dz"), _chk5(y, "y"), _chk5(dy, "dy"), _chk5(z, "z") if z is not None else 0,
        _chk5(dres, "dres") if dres is not None else 0, int(relu), int(training),
        int(dres_accumulate), _stream()), "bn_act_backward")


def bn_act_backward_coeffs(dz, y, scale, shift, mean, invstd, sums_ws, coef, dgamma, dbeta, relu, training):
    """The reduction pass of bn_act_backward and coef[5][C] (A, B, D, scale, shift) of its apply pass, which
    the reader of dy runs itself (conv_wgrad_bn)."""
    N, C_, T, H, W = y.shape
    if sums_ws.numel() < 2 * C_ * N:
        raise ValueError("coclr_amd: bn_act_backward workspace too small")
    if coef.numel() < 5 * C_:
        raise ValueError("coclr_amd: bn_act_backward_coeffs needs 5 x C coefficients")
    _lib.check(_L().coclr_bn_act_backward_coeffs(
        _p(dz), _p(y), _p(scale), _p(shift), _p(mean), _p(invstd), _p(sums_ws, torch.float64), _p(coef),
        _p(dgamma), _p(dbeta), N, C_, T * H * W, _chk5(dz, "dz"), _chk5(y, "y"), int(relu), int(training),
        _stream()), "bn_act_backward_coeffs")


# ---- pooling ---------------------------------------------------------------------

def maxpool_fwd(geom, x, y, indices=None, in_scale=None, in_shift=None, in_relu=False):
    """in_scale / in_shift: per-channel affine (+ ReLU) applied to x as it is read -- the pool then
    consumes the RAW convolution output of the BatchNorm unit in front of it."""
    d = _desc(geom)
    d.x_nstride = _chk5(x, "x")
    d.y_nstride = _chk5(y, "y")
    _lib.check(_L().coclr_maxpool3d_fwd(C.byref(d), _p(x), _p(y), _p(indices, torch.int32),
                                        _p(in_scale), _p(in_shift), int(in_relu), _stream()),
               "maxpool3d_fwd")


def maxpool_bwd(geom, dy, indices, dx, accumulate=False):
    _lib.check(_L().coclr_maxpool3d_bwd(
        C.byref(_desc(geom)), _p(dy), _p(indices, torch.int32), _p(dx), _chk5(dy, "dy"),
        _chk5(dx, "dx"), int(accumulate), _stream()), "maxpool3d_bwd")


def bn_act_backward_pooled(geom, pool_dy, indices, y, scale, shift, mean, invstd, sums_ws, dy, dgamma,
                           dbeta, relu, training):
    """BatchNorm(+ReLU) backward of a unit consumed in fused form by the max-pool `geom`
    (maxpool_fwd with in_scale / in_shift): pool backward, the two BatchNorm reductions and the
    apply pass without ever writing the gradient of the normalised activation."""
    N, C_ = y.shape[0], y.shape[1]
    if sums_ws.numel() < 2 * C_ * N:
        raise ValueError("coclr_amd: bn_act_backward_pooled workspace too small")
    _lib.check(_L().coclr_bn_act_backward_pooled(
        C.byref(_desc(geom)), _p(pool_dy), _p(indices, torch.int32), _p(y), _p(scale), _p(shift),
        _p(mean), _p(invstd), _p(sums_ws, torch.float64), _p(dy), _p(dgamma), _p(dbeta),
        _chk5(pool_dy, "pool_dy"), _chk5(y, "y"), _chk5(dy, "dy"), int(relu), int(training),
        _stream()), "bn_act_backward_pooled")


def pooled_backward_fits(geom):
    """Does bn_act_backward_pooled take this pool?  Asked of the library (the answer depends on the
    kernel's LDS tiling), once per geometry."""
    v = getattr(geom, "_pooled_fits", None)
    if v is None:
        out = C.c_int32(0)
        _lib.check(_L().coclr_bn_act_backward_pooled_fits(C.byref(geom.desc), C.byref(out)),
                   "bn_act_backward_pooled_fits")
        v = bool(out.value)
        try:
            geom._pooled_fits = v
        except AttributeError:
            pass
    return v


def global_avgpool_fwd(x, y):
    planes = x.shape[0] * x.shape[1]
    _lib.check(_L().coclr_global_avgpool_fwd(_p(x), _p(y), planes, x.numel() // planes,
                                                    _stream()), "global_avgpool_fwd")


def global_avgpool_bwd(dy, dx):
    planes = dx.shape[0] * dx.shape[1]
    _lib.check(_L().coclr_global_avgpool_bwd(_p(dy), _p(dx), planes, dx.numel() // planes,
                                                    _stream()), "global_avgpool_bwd")


# ---- head --------------------------------------------------------------------------

def gemm_workspace(M, N, K, splits):
    out = C.c_int64(0)
    _lib.check(_L().coclr_gemm_workspace(M, N, K, splits, C.byref(out)), "gemm_workspace")
    return out.value


def gemm(a, sam, sak, b, sbk, sbn, c, ldc, bias, M, N, K, alpha=1.0, relu=False, accumulate=False,
         splits=1, workspace=None):
    _lib.check(_L().coclr_gemm(
        _p(a), sam, sak, _p(b), sbk, sbn, _p(c), ldc, _p(bias), M, N, K, alpha, int(relu),
        int(accumulate), splits, _p(workspace), _stream()), "gemm")


def gemm_fused_workspace(M, N, K, splits):
    return M * N * max(1, splits)


def gemm_fused(a, sam, sak, b, sbk, sbn, c, ldc, bias, M, N, K, alpha=1.0, relu=False, splits=1,
               workspace=None, mode=0, S=0, ep_a=None, lda=0, ep_b=None, ep_y=None, inv_norm=None, out2=None,
               f=0.0, rowsum=None):
    """coclr_gemm_fused (include/coclr_hip.h): the product with the row-level operation that follows it
    (mode 1 ReLU backward, 2 row normalise, 3 l_pos + normalise backward, 4 average-pool backward) applied
    by the kernel that folds the split-K partials; mode 0 with splits 1 is the plain product in one launch
    (optionally + row sums of A)."""
    ep = _lib.GemmEpilogue(int(mode), int(S), _p(ep_a), int(lda), _p(ep_b), _p(ep_y), _p(inv_norm), _p(out2),
                           float(f), _p(rowsum))
    _lib.check(_L().coclr_gemm_fused(
        _p(a), sam, sak, _p(b), sbk, sbn, _p(c), ldc, _p(bias), M, N, K, alpha, int(relu), splits,
        _p(workspace), C.byref(ep), _stream()), "gemm_fused")


def l2norm_fwd(x, y, inv_norm, eps=1e-12):
    rows, D = x.shape
    _lib.check(_L().coclr_l2norm_fwd(_p(x), _p(y), _p(inv_norm), rows, D, eps, _stream()),
               "l2norm_fwd")


def l2norm_bwd(dy, y, inv_norm, dx):
    rows, D = y.shape
    _lib.check(_L().coclr_l2norm_bwd(_p(dy), _p(y), _p(inv_norm), _p(dx), rows, D,
                                            _stream()), "l2norm_bwd")


def nce_logits_fwd(q, k, queue, logits, T):
    B, D = q.shape
    K = queue.shape[1]
    _lib.check(_L().coclr_nce_logits_fwd(_p(q), _p(k), _p(queue), _p(logits), B, D, K, T,
                                                _stream()), "nce_logits_fwd")


def nce_logits_bwd(dlogits, k, queue, dq, workspace, T, splits):
    B, D = dq.shape
    K = queue.shape[1]
    _lib.check(_L().coclr_nce_logits_bwd(_p(dlogits), _p(k), _p(queue), _p(dq),
                                                _p(workspace), B, D, K, T, splits, _stream()),
               "nce_logits_bwd")


def momentum_update(table, nchunks, m, one_minus_m, pairs=None):
    """`pairs` = (dst tensors, src tensors) the pointer table was built from: not used by the
    kernel; callers pass it so the tensors stay referenced while the launch is queued."""
    _lib.check(_L().coclr_momentum_update(_p(table, torch.int64), nchunks, m, one_minus_m,
                                                 _stream()), "momentum_update")


def queue_enqueue(queue, keys, ptr):
    D, K = queue.shape
    BW = keys.shape[0]
    _lib.check(_L().coclr_queue_enqueue(_p(queue), _p(keys), D, K, BW,
                                               _p(ptr, torch.int64), _stream()), "queue_enqueue")


def queue_fill_i64(queue, vals, const_val, BW, ptr):
    _lib.check(_L().coclr_queue_fill_i64(
        _p(queue, torch.int64), _p(vals, torch.int64), const_val, queue.shape[0], BW,
        _p(ptr, torch.int64), _stream()), "queue_fill_i64")


def queue_advance(ptr, BW, K):
    _lib.check(_L().coclr_queue_advance(_p(ptr, torch.int64), BW, K, _stream()),
               "queue_advance")


def positive_mask(sim, src, names, mask, topk):
    B, K1 = mask.shape
    _lib.check(_L().coclr_positive_mask(
        _p(sim), _p(src, torch.int64), _p(names, torch.int64), _p(mask, torch.uint8), B, K1 - 1,
        topk, _stream()), "positive_mask")


def mine_workspace(B, K, topk, device):
    """(candidate values, candidate columns, zeroed row-tile counters) for mine_positives; the
    counters are left zero by every launch, so one workspace serves a model for its lifetime."""
    nt = (K + 63) // 64
    return (torch.empty(B * nt * max(topk, 1), dtype=torch.float32, device=device),
            torch.empty(B * nt * max(topk, 1), dtype=torch.int32, device=device),
            torch.zeros((B + 31) // 32, dtype=torch.int32, device=device))


def mine_positives(kf, queue_second, src, names, mask, topk, workspace, sim_out=None):
    """mask <- column 0 | same-source columns | top-k of kf @ queue_second over the other columns, in
    one launch (model/pretrain.py:397-413)."""
    B, D = kf.shape
    K = queue_second.shape[1]
    cv, ci, cnt = workspace
    nt = (K + 63) // 64
    if cv.numel() < B * nt * max(topk, 1) or cnt.numel() < (B + 31) // 32:
        raise ValueError("coclr_amd: mine_positives workspace too small")
    _lib.check(_L().coclr_mine_positives(
        _p(kf), _p(queue_second), _p(src, torch.int64), _p(names, torch.int64), _p(mask, torch.uint8),
        _p(cv), _p(ci, torch.int32), _p(cnt, torch.int32), _p(sim_out), B, D, K, topk, _stream()),
        "mine_positives")


def gather_rows(inp, idx, out):
    """out[i] = inp[idx[i]]; `inp` rows must be dense but may be strided along dim 0."""
    rows = out.shape[0]
    row_elems = out.numel() // rows
    if inp.dim() > 1 and inp[0].numel() == row_elems and inp[0].is_contiguous():
        in_stride = inp.stride(0) if inp.shape[0] > 1 else row_elems
    else:
        raise ValueError("coclr_amd: gather_rows needs dense source rows")
    _lib.check(_L().coclr_gather_rows(_p(inp), _p(idx, torch.int64), _p(out), rows,
                                             row_elems, max(in_stride, row_elems), _stream()),
               "gather_rows")


def pull_rows(row_ptrs, out, keep=None):
    """out[i] = row at device address row_ptrs[i] (int64 tensor); `keep`: the (peer) tensors the
    addresses point into, referenced while the launch is queued."""
    rows = out.shape[0]
    _lib.check(_L().coclr_pull_rows(_p(row_ptrs, torch.int64), _p(out), rows, out.numel() // rows,
                                    _stream()), "pull_rows")


def relu_fwd(x, y):
    _lib.check(_L().coclr_relu_fwd(_p(x), _p(y), x.numel(), _stream()), "relu_fwd")


def relu_bwd(dy, y, dx):
    _lib.check(_L().coclr_relu_bwd(_p(dy), _p(y), _p(dx), y.numel(), _stream()), "relu_bwd")


def colsum(x, out):
    rows, cols = x.shape
    _lib.check(_L().coclr_colsum(_p(x), _p(out), rows, cols, _stream()), "colsum")


# ---- S3D-G self gating ---------------------------------------------------------------

def sigmoid_fwd(s_, w):
    _lib.check(_L().coclr_sigmoid_fwd(_p(s_), _p(w), s_.numel(), _stream()), "sigmoid_fwd")


def sigmoid_bwd(dw, w, ds):
    _lib.check(_L().coclr_sigmoid_bwd(_p(dw), _p(w), _p(ds), w.numel(), _stream()), "sigmoid_bwd")


def plane_scale(a, gain, bias, out, accumulate=False):
    """out[n][c][:] (+)= a[n][c][:] * gain[n][c] + bias[n][c]; a / out may be channel slices."""
    N, C_, T, H, W = a.shape
    _lib.check(_L().coclr_plane_scale(_p(a), _p(gain), _p(bias), _p(out), N, C_, T * H * W,
                                      _chk5(a, "a"), _chk5(out, "out"), int(accumulate), _stream()),
               "plane_scale")


def plane_dot(a, b, out):
    """out[n][c] = <a[n][c], b[n][c]> over (T, H, W)."""
    N, C_, T, H, W = a.shape
    _lib.check(_L().coclr_plane_dot(_p(a), _p(b), _p(out), N, C_, T * H * W, _chk5(a, "a"),
                                    _chk5(b, "b"), _stream()), "plane_dot")


# ---- training-loop neighbours: optimiser, loss epilogue, input staging -------------------

def adam_step(table, nchunks, hyper, steps, groups, ngroups, mom_m=0.0, mom_1m=0.0, keep=None):
    """One multi-tensor Adam launch (+ folded momentum-encoder update where the table names a key
    parameter).  `keep`: the tensors the table points at, referenced while the launch is queued."""
    _lib.check(_L().coclr_adam_step(_p(table, torch.int64), nchunks, _p(hyper, torch.float64), _p(steps),
                                    _p(groups, torch.int32), ngroups, mom_m, mom_1m, _stream()),
               "adam_step")


def sgd_step(table, nchunks, hyper, keep=None):
    """One multi-tensor SGD launch (csrc/optim.hip).  `keep`: the tensors the table points at,
    referenced while the launch is queued."""
    _lib.check(_L().coclr_sgd_step(_p(table, torch.int64), nchunks, _p(hyper, torch.float64), _stream()),
               "sgd_step")


def nce_loss_fwd(logits, mask, target, rowstats, flags, scalars, mode, drop_self=False, k1=1, k2=5):
    B, N1 = logits.shape
    _lib.check(_L().coclr_nce_loss_fwd(
        _p(logits), _p(mask, torch.uint8), _p(target, torch.int64), _p(rowstats),
        _p(flags, torch.uint8), _p(scalars), B, N1, mode, int(drop_self), k1, k2, _stream()),
        "nce_loss_fwd")


def nce_loss_bwd(logits, mask, target, rowstats, flags, dloss, dlogits, mode):
    B, N1 = logits.shape
    _lib.check(_L().coclr_nce_loss_bwd(
        _p(logits), _p(mask, torch.uint8), _p(target, torch.int64), _p(rowstats),
        _p(flags, torch.uint8), _p(dloss), _p(dlogits), B, N1, mode, _stream()), "nce_loss_bwd")


def stage_clips(frames, out, S, mean, std):
    """frames (B, C, S*T, H, W) uint8 or fp32 in [0,1] -> out (B, S, C, T, H, W) fp32."""
    B, Cc = frames.shape[0], frames.shape[1]
    thw = frames[0, 0].numel() // S
    if frames.dtype == torch.uint8:
        src, u8 = _p(frames, torch.uint8), 1
    else:
        src, u8 = _p(frames), 0
    m = (C.c_float * Cc)(*[float(v) for v in mean])
    s = (C.c_float * Cc)(*[float(v) for v in std])
    _lib.check(_L().coclr_stage_clips(src, u8, _p(out), B, Cc, S, thw, m, s, _stream()),
               "stage_clips")


def stage_crops(frames, slot_frame, crops, cw, ch, S, xmin, xk, ymin, yk, mean, std, out):
    """frames (F, H, W, 3) uint8, slot_frame (n_clips, T) int32 (validated by the caller: the kernel reads it
    on the device), crops [(x0, y0, flip)] -> out (n_crops, n_clips, 3, T, S, S) fp32.  Tables: xmin (Sp,),
    xk (xtaps, Sp) int32 with Sp = S rounded up to a multiple of 4, the same for y (include/coclr_hip.h)."""
    if frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("coclr_amd: frames must be contiguous (F, H, W, 3), got %s" % (tuple(frames.shape),))
    F, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    n_clips, T = slot_frame.shape
    Sp = (S + 3) & ~3
    if tuple(xmin.shape) != (Sp,) or xk.dim() != 2 or xk.shape[1] != Sp or \
            tuple(ymin.shape) != (Sp,) or yk.dim() != 2 or yk.shape[1] != Sp:
        raise ValueError("coclr_amd: resampling tables must be (Sp,) and (taps, Sp) with Sp = %d" % Sp)
    if tuple(out.shape) != (len(crops), n_clips, 3, T, S, S) or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" %
                         ((len(crops), n_clips, 3, T, S, S), tuple(out.shape)))
    for t in (slot_frame, xmin, xk, ymin, yk):
        if not t.is_contiguous():
            raise ValueError("coclr_amd: stage_crops needs contiguous index and table tensors")
    flat = [int(v) for c in crops for v in c]
    if len(flat) != 3 * len(crops) or not crops:
        raise ValueError("coclr_amd: crops must be (x0, y0, flip) triples")
    box = (C.c_int32 * len(flat))(*flat)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    i32 = torch.int32
    _lib.check(_L().coclr_stage_crops(
        _p(frames, torch.uint8), F, H, W, _p(slot_frame, i32), n_clips, T, box, len(crops), cw, ch, S,
        _p(xmin, i32), _p(xk, i32), xk.shape[0], _p(ymin, i32), _p(yk, i32), yk.shape[0], m, s, _p(out),
        _stream()), "stage_crops")


def resize_crops_u8(frames, slot_frame, crops, cw, ch, S, xmin, xk, ymin, yk, out):
    """stage_crops up to the resized bytes: out (n_crops, n_clips*T, S, S, 3) uint8, one image per slot."""
    if frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("coclr_amd: frames must be contiguous (F, H, W, 3), got %s" % (tuple(frames.shape),))
    F, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    n_clips, T = slot_frame.shape
    Sp = (S + 3) & ~3
    if tuple(xmin.shape) != (Sp,) or xk.dim() != 2 or xk.shape[1] != Sp or \
            tuple(ymin.shape) != (Sp,) or yk.dim() != 2 or yk.shape[1] != Sp:
        raise ValueError("coclr_amd: resampling tables must be (Sp,) and (taps, Sp) with Sp = %d" % Sp)
    if tuple(out.shape) != (len(crops), n_clips * T, S, S, 3) or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" %
                         ((len(crops), n_clips * T, S, S, 3), tuple(out.shape)))
    for t in (slot_frame, xmin, xk, ymin, yk):
        if not t.is_contiguous():
            raise ValueError("coclr_amd: resize_crops_u8 needs contiguous index and table tensors")
    flat = [int(v) for c in crops for v in c]
    if len(flat) != 3 * len(crops) or not crops:
        raise ValueError("coclr_amd: crops must be (x0, y0, flip) triples")
    box = (C.c_int32 * len(flat))(*flat)
    i32 = torch.int32
    _lib.check(_L().coclr_resize_crops_u8(
        _p(frames, torch.uint8), F, H, W, _p(slot_frame, i32), n_clips, T, box, len(crops), cw, ch, S,
        _p(xmin, i32), _p(xk, i32), xk.shape[0], _p(ymin, i32), _p(yk, i32), yk.shape[0], _p(out, torch.uint8),
        _stream()), "resize_crops_u8")


def color_jitter_clips(frames, kinds, params, group_size, T, mean, std, out, host_tables=None):
    """frames (N, H, W, 3) uint8 -> out (N/T, 3, T, H, W) fp32; frame n runs program n // group_size of the
    device tables kinds int32 (G, P) / params fp32 (G, P) (include/coclr_hip.h).  `host_tables`: the same two
    tables on the host, which the entry point validates (read back from the device when not given)."""
    _program_call("color_jitter_clips", frames, kinds, params, group_size, T, mean, std, out, host_tables)


def augment_clips(frames, kinds, params, group_size, T, mean, std, out, host_tables=None):
    """color_jitter_clips with kinds 6 (blur, parameter = PIL's fp32 box radius) and 7 (flip) admitted."""
    _program_call("augment_clips", frames, kinds, params, group_size, T, mean, std, out, host_tables)


def _clip_source(frames, desc, desc_host, fields, ragged):
    """What the four resize wrappers check first: the frames -- (F, H, W, 3), or with `ragged` one flat byte buffer of
    frames that differ in size from clip to clip -- and the descriptors, `fields` words per clip, on the device and on
    the host.  Returns what the entry point takes beside the frames' pointer: F, H, W, or the number of bytes."""
    if ragged:
        if frames.dim() != 1 or frames.dtype != torch.uint8 or not frames.is_contiguous():
            raise ValueError("coclr_amd: ragged frames are one flat contiguous uint8 buffer")
    elif frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("coclr_amd: frames must be contiguous (F, H, W, 3), got %s" % (tuple(frames.shape),))
    if desc.dim() != 2 or desc.shape[1] != fields or desc.shape != desc_host.shape or desc_host.is_cuda or \
            desc_host.dtype != torch.int32 or not desc.is_contiguous() or not desc_host.is_contiguous():
        raise ValueError("coclr_amd: clip descriptors must be contiguous int32 (n_clips, %d), device and host" % fields)
    return (frames.numel(),) if ragged else tuple(frames.shape[:3])


def _resize_boxes(name, ragged, frames, desc, desc_host, xtab, ytab, T, S, out):
    src = _clip_source(frames, desc, desc_host, 14 if ragged else 10, ragged)
    n_clips, T, S = desc.shape[0], int(T), int(S)
    if xtab.dim() != 1 or ytab.dim() != 1 or not xtab.is_contiguous() or not ytab.is_contiguous():
        raise ValueError("coclr_amd: %s needs flat contiguous table buffers" % name)
    if tuple(out.shape) != (n_clips * T, S, S, 3) or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" % ((n_clips * T, S, S, 3), tuple(out.shape)))
    i32 = torch.int32
    _lib.check(getattr(_L(), "coclr_" + name)(
        _p(frames, torch.uint8), *src, _p(desc, i32), C.cast(desc_host.data_ptr(), C.POINTER(C.c_int32)), n_clips,
        T, S, _p(xtab, i32), xtab.numel(), _p(ytab, i32), ytab.numel(), _p(out, torch.uint8), _stream()), name)


def _resize2_boxes(name, ragged, frames, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean, std):
    src = _clip_source(frames, desc, desc_host, 18 if ragged else 14, ragged)
    n_clips, T, size, S = desc.shape[0], int(T), int(size), int(S)
    Sp = (S + 3) & ~3
    if xtab.dim() != 1 or ytab.dim() != 1 or not xtab.is_contiguous() or not ytab.is_contiguous():
        raise ValueError("coclr_amd: %s needs flat contiguous stage-1 table buffers" % name)
    if tab2.dim() != 2 or tab2.shape[0] < 2 or tab2.shape[1] != Sp or not tab2.is_contiguous():
        raise ValueError("coclr_amd: the stage-2 table must be contiguous (1 + taps, %d), got %s" % (Sp, tuple(tab2.shape)))
    u8 = out.dtype == torch.uint8
    if not u8 and (mean is None or std is None):
        raise ValueError("coclr_amd: the fp32 form of %s needs mean and std" % name)
    want = (n_clips * T, S, S, 3) if u8 else (n_clips, 3, T, S, S)
    if tuple(out.shape) != want or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" % (want, tuple(out.shape)))
    m, s = (None, None) if u8 else [(C.c_float * 3)(*[float(v) for v in t]) for t in (mean, std)]
    i32 = torch.int32
    _lib.check(getattr(_L(), "coclr_" + name)(
        _p(frames, torch.uint8), *src, _p(desc, i32), C.cast(desc_host.data_ptr(), C.POINTER(C.c_int32)), n_clips,
        T, size, S, _p(xtab, i32), xtab.numel(), _p(ytab, i32), ytab.numel(), _p(tab2, i32), tab2.numel(),
        tab2.shape[0] - 1, m, s, _p(out, torch.uint8) if u8 else None, None if u8 else _p(out), _stream()), name)


def resize_boxes_u8(frames, desc, desc_host, xtab, ytab, T, S, out):
    """frames (F, H, W, 3) uint8; desc int32 (n_clips, 10) on the device and desc_host, the same on the host
    (include/coclr_hip.h); xtab / ytab the concatenated per-box tables, int32, device -> out (n_clips*T, S, S, 3)
    uint8: every clip's own box of its T frames resized to S x S."""
    _resize_boxes("resize_boxes_u8", False, frames, desc, desc_host, xtab, ytab, T, S, out)


def resize2_boxes(frames, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean=None, std=None):
    """The classifier's crop chain in one launch (include/coclr_hip.h: coclr_resize2_boxes): frames (F, H, W, 3) uint8;
    desc int32 (n_clips, 14) on the device and desc_host, the same on the host; xtab / ytab the clips' stage-1 tables
    one after the other, tab2 (1 + taps2, Sp) the shared size -> S table, all int32 on the device.  `out` uint8
    (n_clips*T, S, S, 3) takes the resized bytes; `out` fp32 (n_clips, 3, T, S, S) takes them normalised with
    `mean` / `std`."""
    _resize2_boxes("resize2_boxes", False, frames, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean, std)


def jpeg_workspace(H, W, ncomp, hs, vs):
    """Bytes per frame of the coefficient and sample-plane workspaces of jpeg_decode (no device needed)."""
    a, b = C.c_int64(0), C.c_int64(0)
    rc = _lib.load().coclr_jpeg_workspace(int(H), int(W), int(ncomp), int(hs), int(vs), C.byref(a), C.byref(b))
    if rc != 0:
        raise ValueError("coclr_amd: no JPEG workspace for %d x %d frames of %d components sampled %d x %d" %
                         (W, H, ncomp, hs, vs))
    return a.value, b.value


def _decode_frames(chunk_bytes, meta, meta_host):
    """What the two decode wrappers check first -> (chunk_bytes, F, width)."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes != 0 and not 8 <= chunk_bytes <= 65536:
        raise ValueError("coclr_amd: chunk_bytes must be 0 or in 8..65536, got %d" % chunk_bytes)
    if meta.dim() != 2 or meta.shape != meta_host.shape or meta_host.is_cuda or meta_host.dtype != torch.int32 or \
            not meta.is_contiguous() or not meta_host.is_contiguous():
        raise ValueError("coclr_amd: frame descriptors must be contiguous int32 (F, width), device and host")
    return (chunk_bytes,) + tuple(meta.shape)


def _check_status(status, F):
    if tuple(status.shape) != (F,) or not status.is_contiguous():
        raise ValueError("coclr_amd: status must be contiguous (%d,), got %s" % (F, tuple(status.shape)))


def jpeg_decode(data, meta, meta_host, H, W, ncomp, hs, vs, coefs, planes, out, status, stages=7, chunk_bytes=0):
    """data uint8 (n,), meta int32 (F, width) on the device and meta_host, the same on the host (include/coclr_hip.h:
    coclr_jpeg_decode) -> out uint8 (F, H, W, 3), status int32 (F,).  coefs int16 / planes uint8: flat workspaces of
    F times jpeg_workspace().  `stages`: 1 entropy, 2 inverse DCT, 4 colour; 7 = all three.  `chunk_bytes`: 0, or
    8..65536 to decode frames without restart markers on a lane per chunk of that many bytes
    (coclr_jpeg_decode_split); the results are the same bit for bit."""
    chunk_bytes, F, width = _decode_frames(chunk_bytes, meta, meta_host)
    cb, pb = jpeg_workspace(H, W, ncomp, hs, vs)
    if data.dim() != 1 or not data.is_contiguous() or coefs.numel() * 2 < F * cb or planes.numel() < F * pb or \
            not coefs.is_contiguous() or not planes.is_contiguous():
        raise ValueError("coclr_amd: jpeg_decode needs flat bytes and workspaces of %d + %d bytes per frame" % (cb, pb))
    if tuple(out.shape) != (F, H, W, 3) or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" % ((F, H, W, 3), tuple(out.shape)))
    _check_status(status, F)
    args = (_p(data, torch.uint8), data.numel(), _p(meta, torch.int32),
            C.cast(meta_host.data_ptr(), C.POINTER(C.c_int32)), F, width, int(H), int(W), int(ncomp), int(hs), int(vs),
            int(stages), _p(coefs, torch.int16), _p(planes, torch.uint8), _p(out, torch.uint8),
            _p(status, torch.int32))
    if chunk_bytes:
        _lib.check(_L().coclr_jpeg_decode_split(*args, chunk_bytes, _stream()), "jpeg_decode_split")
    else:
        _lib.check(_L().coclr_jpeg_decode(*args, _stream()), "jpeg_decode")


JR_FIELDS = 8        # csrc/jpeg_core.h: per frame H, W, components, hs, vs, first block, first output byte, 0


def jpeg_decode_ragged(data, meta, meta_host, geom, geom_host, prefix, prefix_host, coefs, planes, out, status,
                       stages=7, chunk_bytes=0):
    """jpeg_decode for frames that differ in geometry (include/coclr_hip.h: coclr_jpeg_decode_ragged): geom int64
    (F, 8) and prefix int64 (2, F + 1) on the device and the same two on the host; coefs int16 / planes uint8 flat
    workspaces of the same number of blocks; out the flat uint8 buffer every frame's first output byte points into."""
    chunk_bytes, F, width = _decode_frames(chunk_bytes, meta, meta_host)
    for dev, host, want, what in ((geom, geom_host, (F, JR_FIELDS), "geometry table"),
                                  (prefix, prefix_host, (2, F + 1), "prefix arrays")):
        if tuple(dev.shape) != want or tuple(host.shape) != want or host.is_cuda or host.dtype != torch.int64 or \
                not dev.is_contiguous() or not host.is_contiguous():
            raise ValueError("coclr_amd: the %s must be contiguous int64 %s, device and host" % (what, want))
    blocks = min(coefs.numel() // 64, planes.numel() // 64)
    if data.dim() != 1 or not data.is_contiguous() or out.dim() != 1 or not out.is_contiguous() or \
            not coefs.is_contiguous() or not planes.is_contiguous() or blocks < 1:
        raise ValueError("coclr_amd: jpeg_decode_ragged needs flat bytes, flat workspaces and a flat output")
    _check_status(status, F)
    hp = lambda t, ty: C.cast(t.data_ptr(), C.POINTER(ty))                   # noqa: E731
    _lib.check(_L().coclr_jpeg_decode_ragged(
        _p(data, torch.uint8), data.numel(), _p(meta, torch.int32), hp(meta_host, C.c_int32), F, width,
        _p(geom, torch.int64), hp(geom_host, C.c_int64), _p(prefix, torch.int64), hp(prefix_host, C.c_int64),
        int(stages), _p(coefs, torch.int16), _p(planes, torch.uint8), blocks, _p(out, torch.uint8), out.numel(),
        _p(status, torch.int32), chunk_bytes, _stream()), "jpeg_decode_ragged")


JS_FIELDS, JS_TABLE_WORDS, JS_TABLE_PAD, JS_ROW_WORDS = 8, 768, 16, 4     # csrc/jpeg_core.h: JS_*


def jpeg_store_desc(data, frames, frames_host, nframes, tables, tables_host, table_sets, segs, segs_host, nsegs, rows,
                    chunk_bytes, host_bytes=False):
    """The `coclr_jpeg_store` of a store's buffers (include/coclr_hip.h), each on the device with its host copy: data
    uint8 flat, frames int64 (capacity, 8), tables int32 (16 + sets * 768,), segs int32 flat, rows int32 (capacity, 4).
    nframes, table_sets and nsegs say how much of each is filled.  `host_bytes`: data and rows may be host tensors,
    what coclr_jpeg_store_gather alone takes (and only pinned: it asks the runtime)."""
    for dev, host, ty in ((frames, frames_host, torch.int64), (tables, tables_host, torch.int32),
                          (segs, segs_host, torch.int32)):
        if dev.dtype != ty or host.dtype != ty or host.is_cuda or dev.shape != host.shape or \
                not dev.is_contiguous() or not host.is_contiguous():
            raise ValueError("coclr_amd: a store's tables are contiguous, device and host alike")
    if data.dtype != torch.uint8 or data.dim() != 1 or rows.dtype != torch.int32 or not rows.is_contiguous() or \
            frames.shape[0] < nframes or tables.numel() < JS_TABLE_PAD + table_sets * JS_TABLE_WORDS or \
            segs.numel() < nsegs:
        raise ValueError("coclr_amd: a store's buffers do not hold what it says is filled")
    bytes_of = (lambda t, ty: t.data_ptr()) if host_bytes else _p
    return _lib.JpegStore(bytes_of(data, torch.uint8), data.numel(), _p(frames, torch.int64), frames_host.data_ptr(),
                          int(nframes), _p(tables, torch.int32), tables_host.data_ptr(), int(table_sets),
                          _p(segs, torch.int32) if nsegs else None, segs_host.data_ptr() if nsegs else None, int(nsegs),
                          bytes_of(rows, torch.int32), rows.numel() // JS_ROW_WORDS, int(chunk_bytes))


def jpeg_store_index(store, f0, f1):
    """Writes the chunk rows of the restart-less frames among store frames [f0, f1) (include/coclr_hip.h:
    coclr_jpeg_store_index); `store`: the arguments of jpeg_store_desc."""
    desc = jpeg_store_desc(*store)
    _lib.check(_L().coclr_jpeg_store_index(C.byref(desc), int(f0), int(f1), _stream()), "jpeg_store_index")


JW_FIELDS = 4        # csrc/jpeg_core.h: per frame the box x0, y0, w, h


def _jpeg_decode_store(who, store, sel, sel_host, geom, geom_host, window, prefix, prefix_host, coefs, planes, out,
                       status, stages):
    """The body of jpeg_decode_store (`window` None) and jpeg_decode_store_window (`window`: the table, device and
    host)."""
    desc = jpeg_store_desc(*store)
    F = sel_host.numel()
    tables = [(sel, sel_host, (F,), "selection"), (geom, geom_host, (F, JR_FIELDS), "geometry table"),
              (prefix, prefix_host, (3, F + 1), "prefix arrays")]
    if window is not None:
        tables.append(window + ((F, JW_FIELDS), "window table"))
    for dev, host, want, what in tables:
        if tuple(dev.shape) != want or tuple(host.shape) != want or host.is_cuda or host.dtype != torch.int64 or \
                dev.dtype != torch.int64 or not dev.is_contiguous() or not host.is_contiguous():
            raise ValueError("coclr_amd: the %s must be contiguous int64 %s, device and host" % (what, want))
    blocks = min(coefs.numel() // 64, planes.numel() // 64)
    if out.dim() != 1 or not out.is_contiguous() or not coefs.is_contiguous() or not planes.is_contiguous() or \
            blocks < 1:
        raise ValueError("coclr_amd: %s needs flat workspaces and a flat output" % who)
    _check_status(status, F)
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))                # noqa: E731
    head = (C.byref(desc), _p(sel, torch.int64), hp(sel_host), F, _p(geom, torch.int64), hp(geom_host))
    tail = (_p(prefix, torch.int64), hp(prefix_host), int(stages), _p(coefs, torch.int16), _p(planes, torch.uint8),
            blocks, _p(out, torch.uint8), out.numel(), _p(status, torch.int32), _stream())
    if window is None:
        _lib.check(_L().coclr_jpeg_decode_store(*head, *tail), who)
    else:
        _lib.check(_L().coclr_jpeg_decode_store_window(*head, _p(window[0], torch.int64), hp(window[1]), *tail), who)


def jpeg_decode_store(store, sel, sel_host, geom, geom_host, prefix, prefix_host, coefs, planes, out, status, stages=7):
    """jpeg_decode_ragged for the store frames `sel` names (include/coclr_hip.h: coclr_jpeg_decode_store): sel int64
    (F,), geom int64 (F, 8) and prefix int64 (3, F + 1) -- blocks, row groups, entropy lanes -- on the device and the
    same three on the host; `store`: the arguments of jpeg_store_desc; workspaces and output as jpeg_decode_ragged."""
    _jpeg_decode_store("jpeg_decode_store", store, sel, sel_host, geom, geom_host, None, prefix, prefix_host, coefs,
                       planes, out, status, stages)


def jpeg_decode_store_window(store, sel, sel_host, geom, geom_host, window, window_host, prefix, prefix_host, coefs,
                             planes, out, status, stages=7):
    """jpeg_decode_store for one pixel box of every frame (include/coclr_hip.h: coclr_jpeg_decode_store_window):
    window int64 (F, 4) -- x0, y0, w, h -- on the device and the host; frame i of `out` is its h x w box at geom[i, 6];
    the first two rows of `prefix` count the box's MCU rectangle and row groups; the workspaces keep the full-frame
    layout."""
    _jpeg_decode_store("jpeg_decode_store_window", store, sel, sel_host, geom, geom_host, (window, window_host), prefix,
                       prefix_host, coefs, planes, out, status, stages)


JG_FIELDS = 8        # csrc/jpeg_core.h: per distinct frame of a gather, JG_*


def jpeg_store_gather(store, plan, plan_host, slot_host, frames_host, arena, arena_rows):
    """Copies the hulls and rows of the distinct frames `plan` names from a store whose bytes and rows may be pinned host
    memory to the device arenas (include/coclr_hip.h: coclr_jpeg_store_gather): plan int64 (m, 8) on the device and
    plan_host; slot_host int64 (n,) and frames_host int64 (n, 8), the plan entry and the rebased record of each frame
    of the decode call; arena uint8 flat and arena_rows int32 (rows, 4) on the device.  `store`: the arguments of
    jpeg_store_desc."""
    desc = jpeg_store_desc(*store, host_bytes=True)
    m, n = plan_host.shape[0], slot_host.numel()
    for t, want, what in ((plan, (m, JG_FIELDS), "plan"), (plan_host, (m, JG_FIELDS), "plan"),
                          (slot_host, (n,), "slots"), (frames_host, (n, JS_FIELDS), "rebased records")):
        if tuple(t.shape) != want or t.dtype != torch.int64 or not t.is_contiguous() or \
                (t is not plan and t.is_cuda):
            raise ValueError("coclr_amd: the %s of a gather must be contiguous int64 %s" % (what, want))
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous() or \
            arena_rows.dtype != torch.int32 or not arena_rows.is_contiguous():
        raise ValueError("coclr_amd: jpeg_store_gather needs a flat uint8 arena and int32 rows")
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))                # noqa: E731
    rc = _L().coclr_jpeg_store_gather(C.byref(desc), _p(plan, torch.int64), hp(plan_host), m, hp(slot_host),
                                      hp(frames_host), n, _p(arena, torch.uint8), arena.numel(),
                                      _p(arena_rows, torch.int32), arena_rows.numel() // JS_ROW_WORDS, _stream())
    _lib.check(rc, "jpeg_store_gather")


JG_MAX_SHARDS = 8    # csrc/jpeg_core.h: the sources of one sharded gather, one per GPU of a node


def jpeg_shard_desc(data, rows, frames_host, nframes, tables_host, table_sets, segs_host, nsegs, chunk_bytes):
    """The `coclr_jpeg_store` of ONE SOURCE of jpeg_store_gather_shards: data uint8 flat and rows int32 (capacity, 4),
    on the device (this process's memory or a peer's mapped buffer) or pinned on the host; the host tables the shard's
    records are read against: frames_host int64 (>= nframes, 8), tables_host int32, segs_host int32.  The device
    tables of a store are not part of a source; a shard may hold no frame."""
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous() or rows.dtype != torch.int32 or \
            not rows.is_contiguous() or rows.numel() % JS_ROW_WORDS:
        raise ValueError("coclr_amd: a shard's bytes are flat uint8 and its rows contiguous int32 (n, 4)")
    for host, ty in ((frames_host, torch.int64), (tables_host, torch.int32), (segs_host, torch.int32)):
        if host.dtype != ty or host.is_cuda or not host.is_contiguous():
            raise ValueError("coclr_amd: a shard's tables are contiguous host tensors")
    if frames_host.numel() < nframes * JS_FIELDS or tables_host.numel() < JS_TABLE_PAD + table_sets * JS_TABLE_WORDS or \
            segs_host.numel() < nsegs:
        raise ValueError("coclr_amd: a shard's tables do not hold what it says is filled")
    return _lib.JpegStore(data.data_ptr(), data.numel(), None, frames_host.data_ptr() if nframes else None,
                          int(nframes), None, tables_host.data_ptr(), int(table_sets), None,
                          segs_host.data_ptr() if nsegs else None, int(nsegs), rows.data_ptr(),
                          rows.numel() // JS_ROW_WORDS, int(chunk_bytes))


def jpeg_store_gather_shards(shards, plan, plan_host, shard, shard_host, slot_host, frames_host, arena, arena_rows):
    """jpeg_store_gather over several sources (include/coclr_hip.h: coclr_jpeg_store_gather_shards): `shards` the
    arguments of jpeg_shard_desc per source, 1..8 of them; plan int64 (m, 8) and shard int64 (m,) on the device with
    plan_host and shard_host; the rest as jpeg_store_gather."""
    if not 1 <= len(shards) <= JG_MAX_SHARDS:
        raise ValueError("coclr_amd: a sharded gather has 1..%d sources, got %d" % (JG_MAX_SHARDS, len(shards)))
    descs = [jpeg_shard_desc(*s) for s in shards]
    m, n = plan_host.shape[0], slot_host.numel()
    for t, want, what in ((plan, (m, JG_FIELDS), "plan"), (plan_host, (m, JG_FIELDS), "plan"),
                          (shard, (m,), "shard column"), (shard_host, (m,), "shard column"),
                          (slot_host, (n,), "slots"), (frames_host, (n, JS_FIELDS), "rebased records")):
        if tuple(t.shape) != want or t.dtype != torch.int64 or not t.is_contiguous() or \
                (t is not plan and t is not shard and t.is_cuda):
            raise ValueError("coclr_amd: the %s of a gather must be contiguous int64 %s" % (what, want))
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous() or \
            arena_rows.dtype != torch.int32 or not arena_rows.is_contiguous():
        raise ValueError("coclr_amd: jpeg_store_gather_shards needs a flat uint8 arena and int32 rows")
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))                # noqa: E731
    table = (C.POINTER(_lib.JpegStore) * len(descs))(*[C.pointer(d) for d in descs])
    rc = _L().coclr_jpeg_store_gather_shards(table, len(descs), _p(plan, torch.int64), hp(plan_host),
                                             _p(shard, torch.int64), hp(shard_host), m, hp(slot_host), hp(frames_host),
                                             n, _p(arena, torch.uint8), arena.numel(), _p(arena_rows, torch.int32),
                                             arena_rows.numel() // JS_ROW_WORDS, _stream())
    _lib.check(rc, "jpeg_store_gather_shards")


def resize_boxes_ragged_u8(pixels, desc, desc_host, xtab, ytab, T, S, out):
    """resize_boxes_u8 over a flat byte buffer of frames that differ in size from clip to clip: desc int32
    (n_clips, 14), the ten words of resize_boxes_u8 then {offset low, offset high, W, H} of the clip's frames
    (include/coclr_hip.h: coclr_resize_boxes_ragged_u8)."""
    _resize_boxes("resize_boxes_ragged_u8", True, pixels, desc, desc_host, xtab, ytab, T, S, out)


def resize2_boxes_ragged(pixels, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean=None, std=None):
    """resize2_boxes over a flat byte buffer of frames that differ in size from clip to clip: desc int32 (n_clips, 18),
    the fourteen words of resize2_boxes then {offset low, offset high, W, H} (include/coclr_hip.h:
    coclr_resize2_boxes_ragged)."""
    _resize2_boxes("resize2_boxes_ragged", True, pixels, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean, std)


def stage_crops_ragged(pixels, desc, desc_host, slot_off, slot_off_host, cw, ch, S, xmin, xk, ymin, yk, out, mean=None,
                       std=None):
    """stage_crops / resize_crops_u8 for the clips of many videos in one launch (include/coclr_hip.h:
    coclr_stage_crops_ragged): pixels the flat byte buffer; desc int32 (n_clips, 5) = {x0, y0, flip, W, H} and slot_off
    int64 (n_clips, T), the byte offset of every slot's frame, each on the device and on the host; the tables as
    stage_crops takes them.  `out` fp32 (n_clips, 3, T, S, S) takes the clips normalised with `mean` / `std`; `out`
    uint8 (n_clips*T, S, S, 3) takes the resized bytes."""
    _clip_source(pixels, desc, desc_host, 5, True)
    n_clips, S = desc.shape[0], int(S)
    if slot_off.dim() != 2 or slot_off.shape[0] != n_clips or slot_off.shape != slot_off_host.shape or \
            slot_off_host.is_cuda or slot_off_host.dtype != torch.int64 or not slot_off.is_contiguous() or \
            not slot_off_host.is_contiguous():
        raise ValueError("coclr_amd: slot offsets must be contiguous int64 (n_clips, T), device and host")
    T = slot_off.shape[1]
    Sp = (S + 3) & ~3
    if tuple(xmin.shape) != (Sp,) or xk.dim() != 2 or xk.shape[1] != Sp or \
            tuple(ymin.shape) != (Sp,) or yk.dim() != 2 or yk.shape[1] != Sp:
        raise ValueError("coclr_amd: resampling tables must be (Sp,) and (taps, Sp) with Sp = %d" % Sp)
    for t in (xmin, xk, ymin, yk):
        if not t.is_contiguous():
            raise ValueError("coclr_amd: stage_crops_ragged needs contiguous table tensors")
    u8 = out.dtype == torch.uint8
    if not u8 and (mean is None or std is None):
        raise ValueError("coclr_amd: the fp32 form of stage_crops_ragged needs mean and std")
    want = (n_clips * T, S, S, 3) if u8 else (n_clips, 3, T, S, S)
    if tuple(out.shape) != want or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" % (want, tuple(out.shape)))
    m, s = (None, None) if u8 else [(C.c_float * 3)(*[float(v) for v in t]) for t in (mean, std)]
    i32 = torch.int32
    _lib.check(_L().coclr_stage_crops_ragged(
        _p(pixels, torch.uint8), pixels.numel(), _p(desc, i32), C.cast(desc_host.data_ptr(), C.POINTER(C.c_int32)),
        n_clips, T, _p(slot_off, torch.int64), C.cast(slot_off_host.data_ptr(), C.POINTER(C.c_int64)), int(cw), int(ch),
        S, _p(xmin, i32), _p(xk, i32), xk.shape[0], _p(ymin, i32), _p(yk, i32), yk.shape[0], m, s,
        _p(out, torch.uint8) if u8 else None, None if u8 else _p(out), _stream()), "stage_crops_ragged")


def _program_call(name, frames, kinds, params, group_size, T, mean, std, out, host_tables):
    if frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("coclr_amd: frames must be contiguous (N, H, W, 3), got %s" % (tuple(frames.shape),))
    N, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    if kinds.dim() != 2 or kinds.shape != params.shape or not kinds.is_contiguous() or not params.is_contiguous():
        raise ValueError("coclr_amd: kinds and params must be contiguous (G, P) tables, got %s and %s" %
                         (tuple(kinds.shape), tuple(params.shape)))
    G, P = kinds.shape
    T = int(T)
    if T < 1 or N % T != 0:
        raise ValueError("coclr_amd: %d frames do not make clips of %d" % (N, T))
    if tuple(out.shape) != (N // T, 3, T, H, W) or not out.is_contiguous():
        raise ValueError("coclr_amd: out must be contiguous %s, got %s" % ((N // T, 3, T, H, W), tuple(out.shape)))
    hk, hp = host_tables if host_tables is not None else (kinds.cpu(), params.cpu())
    if hk.shape != kinds.shape or hp.shape != params.shape or hk.is_cuda or hp.is_cuda or \
            not hk.is_contiguous() or not hp.is_contiguous() or hk.dtype != torch.int32 or hp.dtype != torch.float32:
        raise ValueError("coclr_amd: host_tables must be contiguous host copies of kinds and params")
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(getattr(_L(), "coclr_" + name)(
        _p(frames, torch.uint8), N, H, W, T, _p(kinds, torch.int32), _p(params),
        C.cast(hk.data_ptr(), C.POINTER(C.c_int32)), C.cast(hp.data_ptr(), C.POINTER(C.c_float)), G, P,
        int(group_size), m, s, _p(out), _stream()), name)


# ---- evaluation consumers ---------------------------------------------------------------

def colstats_workspace(rows, cols):
    out = C.c_int64(0)
    _lib.check(_L().coclr_colstats_workspace(rows, cols, C.byref(out)), "colstats_workspace")
    return out.value


def bn1d_stats(x, stats, workspace):
    rows, cols = x.shape
    _lib.check(_L().coclr_bn1d_stats(_p(x), _p(stats), _p(workspace), rows, cols, _stream()),
               "bn1d_stats")


def center_rows(x, out, workspace):
    rows, cols = x.shape
    _lib.check(_L().coclr_center_rows(_p(x), _p(out), _p(workspace), rows, cols, _stream()),
               "center_rows")


def retrieval_hits(sim, train_label, test_label, ks, hits, topidx=None):
    """ks: int32 device tensor, ascending; hits fp32 (B, len(ks)); topidx int32 (B, ks[-1])."""
    B, N = sim.shape
    if topidx is None:
        raise ValueError("coclr_amd: retrieval_hits needs the topidx buffer (B, kmax)")
    kmax = int(topidx.shape[1])
    _lib.check(_L().coclr_retrieval_hits(
        _p(sim), _p(train_label, torch.int64), _p(test_label, torch.int64), _p(ks, torch.int32),
        ks.shape[0], _p(hits), _p(topidx, torch.int32), B, N, kmax, _stream()),
        "retrieval_hits")


def fuse_scores(p1, p2, labels, fused, argmax, hits):
    """fused (V, C) float64 = (p1 + p2) / 2 in double; argmax int32 (V, 3) = first maximum of p1, p2 and the mean;
    hits fp32 (V, 3) = argmax == labels (eval/merge_2stream_prob.py:80-98).  Everything dense."""
    if p1.dim() != 2 or p2.shape != p1.shape or p1.numel() == 0:
        raise ValueError("coclr_amd: fuse_scores takes two (V, C) probability matrices of one shape")
    V, C_ = p1.shape
    if tuple(labels.shape) != (V,) or tuple(fused.shape) != (V, C_) or tuple(argmax.shape) != (V, 3) or \
            tuple(hits.shape) != (V, 3):
        raise ValueError("coclr_amd: fuse_scores takes labels (V,), fused (V, C), argmax (V, 3) and hits (V, 3)")
    if not all(t.is_contiguous() for t in (p1, p2, labels, fused, argmax, hits)):
        raise ValueError("coclr_amd: fuse_scores takes contiguous tensors")
    _lib.check(_L().coclr_fuse_scores(_p(p1), _p(p2), _p(labels, torch.int64), _p(fused, torch.float64),
                                      _p(argmax, torch.int32), _p(hits), V, C_, _stream()), "fuse_scores")


SEGMENT_MAX_C = 4096      # widest row the segmented accumulate takes (COCLR_SEG_MAX_C)


def _segment_call(name, x, segs, weight, out):
    R, C_ = x.shape
    V = out.shape[0]
    if out.dim() != 2 or out.shape[1] != C_ or not x.is_contiguous() or not out.is_contiguous():
        raise ValueError("coclr_amd: %s takes dense (R, C) rows and a dense (V, C) output" % name)
    if not 1 <= C_ <= SEGMENT_MAX_C:
        raise ValueError("coclr_amd: %s takes rows of 1..%d columns, got %d" % (name, SEGMENT_MAX_C, C_))
    segs = [tuple(int(v) for v in sg) for sg in segs]
    weight = [float(w) for w in weight]
    S = len(segs)
    if S == 0 or len(weight) != S or any(len(sg) != 3 for sg in segs):
        raise ValueError("coclr_amd: %s needs S >= 1 segments (first row, rows, out row) and S weights" % name)
    seg_arr = (C.c_int32 * (3 * S))(*[v for sg in segs for v in sg])
    w_arr = (C.c_float * S)(*weight)
    _lib.check(getattr(_L(), "coclr_" + name)(_p(x), seg_arr, w_arr, _p(out), R, C_, S, V, _stream()), name,
               segs)


def segment_softmax_accum(logits, segs, weight, out):
    """out[o] += weight[s] * sum_{rows of s} softmax(logits[row]) for every segment s = (first row, rows, o).
    `segs` and `weight` are HOST sequences; nothing is copied to the device and nothing synchronises."""
    _segment_call("segment_softmax_accum", logits, segs, weight, out)


def segment_accum(x, segs, weight, out):
    """segment_softmax_accum without the softmax (per-video feature sums)."""
    _segment_call("segment_accum", x, segs, weight, out)


# ---- host-only plan queries of the staging launchers (ABI 26) ---------------------------------------------------
# Each runs its launcher's own validation and planning function and launches nothing; no device is needed.  Device
# pointers are not read, only tested for null and alignment, so the queries take ADDRESSES: PLAN_ADDR (aligned) unless
# the caller names the tensors it will launch with (`t.data_ptr()`).  A refusal raises as the launcher's would.

PLAN_ADDR = 1 << 20


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _band_dict(out):
    return dict(R=out[0], bands=out[1], cap_rows=out[2], lds=out[3], clipped=bool(out[4]), u8out=bool(out[5]),
                ragged=bool(out[6]), vec=bool(out[7]))


def _host_i32(t, fields):
    t = torch.as_tensor(t, dtype=torch.int32).contiguous()
    if t.dim() != 2 or t.shape[1] != fields or t.is_cuda:
        raise ValueError("coclr_amd: host descriptors must be int32 (n_clips, %d)" % fields)
    return t


def stage_crops_plan(F, H, W, n_clips, T, crops, cw, ch, S, xtaps, ytaps, u8=False, out_addr=PLAN_ADDR,
                     mean=(0., 0., 0.), std=(1., 1., 1.)):
    """What stage_crops (u8=False) / resize_crops_u8 (u8=True) would launch: R, bands, cap_rows, lds, clipped, u8out,
    ragged, vec (include/coclr_hip.h: coclr_stage_crops_plan)."""
    flat = [int(v) for c in crops for v in c]
    box = (C.c_int32 * max(len(flat), 1))(*flat)
    out = (C.c_int32 * 8)()
    a = PLAN_ADDR
    _lib.check(_L().coclr_stage_crops_plan(a, F, H, W, a, n_clips, T, box, len(flat) // 3, cw, ch, S, a, a, xtaps, a, a,
                                           ytaps, _f3(mean), _f3(std), out_addr if u8 else None,
                                           None if u8 else out_addr, out), "stage_crops_plan")
    return _band_dict(out)


def stage_crops_ragged_plan(nbytes, desc_host, slot_off_host, cw, ch, S, xtaps, ytaps, u8=False, out_addr=PLAN_ADDR,
                            mean=(0., 0., 0.), std=(1., 1., 1.)):
    """What stage_crops_ragged would launch; desc_host int32 (n_clips, 5), slot_off_host int64 (n_clips, T)."""
    d = _host_i32(desc_host, 5)
    so = torch.as_tensor(slot_off_host, dtype=torch.int64).contiguous()
    out = (C.c_int32 * 8)()
    a = PLAN_ADDR
    _lib.check(_L().coclr_stage_crops_ragged_plan(
        a, int(nbytes), a, C.cast(d.data_ptr(), C.POINTER(C.c_int32)), d.shape[0], so.shape[1], a,
        C.cast(so.data_ptr(), C.POINTER(C.c_int64)), cw, ch, S, a, a, xtaps, a, a, ytaps, _f3(mean), _f3(std),
        out_addr if u8 else None, None if u8 else out_addr, out), "stage_crops_ragged_plan")
    return _band_dict(out)


def resize_boxes_plan(desc_host, T, S, xlen, ylen, shape=None, nbytes=None):
    """What resize_boxes_u8 (shape = (F, H, W)) / resize_boxes_ragged_u8 (nbytes) would launch."""
    ragged = nbytes is not None
    d = _host_i32(desc_host, 14 if ragged else 10)
    F, H, W = (0, 0, 0) if ragged else shape
    out = (C.c_int32 * 8)()
    a = PLAN_ADDR
    _lib.check(_L().coclr_resize_boxes_plan(int(ragged), a, int(nbytes or 0), F, H, W, a,
                                            C.cast(d.data_ptr(), C.POINTER(C.c_int32)), d.shape[0], T, S, a, xlen, a,
                                            ylen, a, out), "resize_boxes_plan")
    return _band_dict(out)


def resize2_boxes_plan(desc_host, T, size, S, xlen, ylen, taps2, u8=False, shape=None, nbytes=None,
                       out_addr=PLAN_ADDR, mean=(0., 0., 0.), std=(1., 1., 1.)):
    """What resize2_boxes (shape = (F, H, W)) / resize2_boxes_ragged (nbytes) would launch: R, bands, cap1, capA, lds,
    one ("h1" | "h2": which rows sized the shared buffer), optin, u8out, ragged, vec."""
    ragged = nbytes is not None
    d = _host_i32(desc_host, 18 if ragged else 14)
    F, H, W = (0, 0, 0) if ragged else shape
    Sp = (S + 3) & ~3
    out = (C.c_int32 * 10)()
    a = PLAN_ADDR
    _lib.check(_L().coclr_resize2_boxes_plan(
        int(ragged), a, int(nbytes or 0), F, H, W, a, C.cast(d.data_ptr(), C.POINTER(C.c_int32)), d.shape[0], T, size,
        S, a, xlen, a, ylen, a, Sp * (1 + taps2), taps2, _f3(mean), _f3(std), out_addr if u8 else None,
        None if u8 else out_addr, out), "resize2_boxes_plan")
    return dict(R=out[0], bands=out[1], cap1=out[2], capA=out[3], lds=out[4], one="h1" if out[5] else "h2",
                optin=bool(out[6]), u8out=bool(out[7]), ragged=bool(out[8]), vec=bool(out[9]))


def stage_clips_plan(B, Cc, S, thw, u8, src_addr=PLAN_ADDR, out_addr=PLAN_ADDR):
    """What stage_clips would launch: u8, vec (16-byte loads and stores), gx."""
    m = (C.c_float * Cc)(*([0.] * Cc)) if 0 < Cc <= 4 else _f3((0, 0, 0))
    s = (C.c_float * Cc)(*([1.] * Cc)) if 0 < Cc <= 4 else _f3((1, 1, 1))
    out = (C.c_int32 * 3)()
    _lib.check(_L().coclr_stage_clips_plan(src_addr, int(bool(u8)), out_addr, B, Cc, S, thw, m, s, out),
               "stage_clips_plan")
    return dict(u8=bool(out[0]), vec=bool(out[1]), gx=out[2])


def jitter_plan(aug, N, H, W, T, kinds_host, params_host, group_size, out_addr=PLAN_ADDR):
    """What color_jitter_clips (aug=False) / augment_clips (aug=True) would launch: aug, use_lds, lds, items,
    per_lane, vec, cuts (contrast and blur ops of the longest program)."""
    hk = torch.as_tensor(kinds_host, dtype=torch.int32).contiguous()
    hp = torch.as_tensor(params_host, dtype=torch.float32).contiguous()
    if hk.dim() != 2 or hk.shape != hp.shape:
        raise ValueError("coclr_amd: kinds and params must be (G, P) tables")
    out = (C.c_int32 * 7)()
    a = PLAN_ADDR
    _lib.check(_L().coclr_jitter_plan(int(bool(aug)), a, N, H, W, T, a, a, C.cast(hk.data_ptr(), C.POINTER(C.c_int32)),
                                      C.cast(hp.data_ptr(), C.POINTER(C.c_float)), hk.shape[0], hk.shape[1],
                                      int(group_size), _f3((0, 0, 0)), _f3((1, 1, 1)), out_addr, out), "jitter_plan")
    return dict(aug=bool(out[0]), use_lds=bool(out[1]), lds=out[2], items=out[3], per_lane=out[4], vec=bool(out[5]),
                cuts=out[6])
