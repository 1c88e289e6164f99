"""Host-to-host clip pipeline behind ``WindowRunner.run_clip_u8``.  ``EdgeSpec``: what a run asks of its edge, one immutable record, checked once, that
keys the cached pipeline.  ``FrameSlots``: a ring of device frame slots (``residency_order``: the order in which a batch's frames become resident).  One
edge object per format, ``BgrEdge`` (BGR frames in and out) or ``y4m_edge.Y4mEdge`` (Y4M payloads in and out, every window on its own plan), with the
same methods.  Per run: ``attach`` the host frames, then ``begin``, which names the frames to make resident first.  Per batch: ``around`` names the
frames needed besides its windows', ``upload`` copies one frame into a slot and ``uploaded`` follows the copies (h2d stream), ``run`` computes
(compute stream), ``d2h`` copies the outputs to pinned memory (d2h stream), ``drain`` hands them to the sink; what ``run`` returns goes to ``d2h`` /
``drain``; after the last batch ``flush`` names what the edge still holds back (None, or what a ``y4m_edge.Stage`` behind the gather flushed: the odd
last frame of an interlaced ``--dedup`` run), which takes the same way out. ``ClipPipeline`` is the double-buffered batch loop.  A runner of tiles (``WindowRunner(tiles=plan)``, ``demfi_amd.tiling``) has the tile's
size while the slots and the outputs keep the frame's: ``Tiler`` crops every uploaded frame into its tiles once, each (run, tile) pair is one run, and
one stitch launch per batch pastes the kept rectangles into the full-size outputs.  16-bit frames are not cropped or stitched (``TileGrid``): their
ingest and egress kernels address a tile inside the full frames."""
import itertools
import weakref
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from . import bitdepth as BD
from . import cadence as K
from . import colour as CL
from . import deint as I
from . import denoise as DN
from . import grain as GR
from . import interlace as IL
from . import lut3d as LU
from . import retime as R
from . import scale as SC
from . import scene as S
from . import shutter as SH
from .y4m_edge import TileGrid, Y4mEdge, consecutive, fill_sink_records, max_runs    # noqa: F401  (fill_sink_records: for the runner)


def deint_conflict(mode, has_fields, has_dedup):
    """Why the deinterlacing ``mode`` cannot run, or None: 'mode' (not one of ``deint.MODES``); other than 'bob' it needs 'fields', and
    no 'dedup' (repeated frames are staged and discarded one field at a time, the other modes need fields of lookahead)."""
    if mode not in I.MODES:
        return 'mode'
    if mode != 'bob' and (has_dedup or not has_fields):
        return 'dedup' if has_fields else 'fields'


_EdgeFields = namedtuple('EdgeSpec', 'y4m cuts full depth layout dedup fields deint_mode', defaults=(False, False, False, 8, '420', None, None, 'bob'))


class EdgeSpec(_EdgeFields):
    """What a run of ``WindowRunner.run_clip_u8`` asks of its edge (default: the BGR edge).  ``y4m``: the Y4M edge; ``cuts``: scene cuts are detected;
    ``full``: the full-length timeline; ``depth``: bits per sample; ``layout``: one of ``y4m.LAYOUTS``; ``dedup``: None or (hi, lo, frac, max_hold);
    ``fields``: None or the field order 't' / 'b' of an interlaced input; ``deint_mode``: one of ``deint.MODES``; ``shutter``: None or (S, D) of a
    synthesized shutter (``demfi_amd.shutter``); ``interlace``: None or (field order 't' / 'b', low-pass mode) of interlaced output
    (``demfi_amd.interlace``); ``scale``: None or (w, h, filter) of resized output (``demfi_amd.scale``); ``depths``: None or (input depth,
    working depth, output depth, dither mode or None) of a run that changes the bit depth (``demfi_amd.bitdepth``): ``depth`` and ``hi`` then
    mean the WORKING depth, the payloads come in at the input's and leave at the output's; three equal depths are None;
    ``shutter_window``: None (the box) or 'triangle', the weights of a shutter's mix (``shutter.window_weights``; only with ``shutter``);
    ``denoise``: None or (A, B, R) of the temporal denoiser in front of the network (``demfi_amd.denoise``: thresholds at the 8-bit scale, frames
    on each side), kept beside the tuple like the others;
    ``colour``: None or (transfer of ``colour.TRANSFERS`` or None, output matrix 'bt601' / 'bt709' or None, output full range or None) of
    ``demfi_amd.colour``: linear light for the mix and the scaler, and the matrix and range written where they differ from the input's
    (three times None is None), kept beside the tuple like ``scale`` and ``denoise``.
    ``grain``: None or (S16, r, C16, curve, seed) of the film grain added behind the encode and in front of the weave (``demfi_amd.grain``),
    kept beside the tuple like ``denoise`` and ``colour``; S16 = 0 is None.  ``deblock``: None or (A, B) of the deblocking filter at the top of the
    ingest (``demfi_amd.deblock``: thresholds at the 8-bit scale), kept beside the tuple like ``denoise``; A = 0, the identity, is None.  ``dering``: None or (P, S, D) of the deringing filter behind the deblocker
    (``demfi_amd.dering``: strengths at the 8-bit scale), kept beside the tuple like ``deblock``; P = S = 0, the identity, is None.  ``deband``: None or (T, R) of the debanding filter behind the deringing filter
    (``demfi_amd.deband``: threshold at the 8-bit scale, radius in samples), kept beside the tuple like ``dering``; T = 0, the identity, is None.
    ``lut``: None or the ``lut3d.Cube`` of the 3D colour LUT applied between the scaler and the encode (``demfi_amd.lut3d``), kept beside the tuple
    like ``grain``; it compares and hashes by its size and its quantised numbers.  ``nlmeans``: None or (S, P, R) of the spatial denoiser between the deringing filter and the debander
    (``demfi_amd.nlmeans``: strength at the 8-bit scale, patch and search radius in samples), kept beside the tuple like ``deband``; S = 0, the identity, is None.  ``reach``: how far the frames an ingest stage reads lie from the frame it writes.
    Hashable: (batch, spec) is what a cached ``ClipPipeline`` can be reused for.
    ``shutter``, ``interlace``, ``scale``, ``depths``, ``shutter_window``, ``denoise``, ``colour``, ``grain``, ``deblock``, ``dering``, ``deband``, ``lut`` and ``nlmeans`` come last and by keyword only, and they are kept beside the tuple's eight items, not among them: a spec
    without them is, item for item, the record it was before there were any, and one with any of them equals no plain tuple.  What the namedtuple makes
    from its items alone does not know them: ``_make``, ``_asdict`` and pickling drop them; the constructor, ``of`` and ``_replace`` are the ways to a spec."""
    shutter = None
    interlace = None
    scale = None
    depths = None
    shutter_window = None
    denoise = None
    colour = None
    grain = None
    deblock = None
    dering = None
    deband = None
    lut = None
    nlmeans = None

    def __new__(cls, *args, shutter=None, interlace=None, scale=None, depths=None, shutter_window=None, denoise=None, colour=None, grain=None,
                deblock=None, dering=None, deband=None, lut=None, nlmeans=None, **kw):
        self = super().__new__(cls, *args, **kw)
        if nlmeans is not None and int(nlmeans[0]) != 0:                  # S = 0 changes nothing: the spec without the field
            self.nlmeans = tuple(int(v) for v in nlmeans)
        if lut is not None:
            self.lut = lut
        if deband is not None and int(deband[0]) != 0:                    # T = 0 changes nothing: the spec without the field
            self.deband = tuple(int(v) for v in deband)
        if dering is not None and (int(dering[0]) != 0 or int(dering[1]) != 0):     # P = S = 0 changes nothing: the spec without the field
            self.dering = tuple(int(v) for v in dering)
        if deblock is not None and int(deblock[0]) != 0:                  # A = 0 changes nothing: the spec without the field
            self.deblock = tuple(int(v) for v in deblock)
        if grain is not None and int(grain[0]) != 0:                      # no strength is the spec without the field
            self.grain = (int(grain[0]), int(grain[1]), int(grain[2]), grain[3], int(grain[4]))
        if colour is not None and any(v is not None for v in colour):     # three times None is the spec without the field
            self.colour = (colour[0], colour[1], None if colour[2] is None else bool(colour[2]))
        if denoise is not None:
            self.denoise = tuple(int(v) for v in denoise)
        if shutter_window not in (None, 'box'):      # the box is the spec without the field
            self.shutter_window = shutter_window
        if shutter is not None:
            self.shutter = (int(shutter[0]), int(shutter[1]))
        if interlace is not None:
            self.interlace = tuple(interlace)
        if scale is not None:
            self.scale = (int(scale[0]), int(scale[1]), scale[2])
        if not BD.is_noop(depths):
            self.depths = (int(depths[0]), int(depths[1]), int(depths[2]), depths[3])
        return self

    def _replace(self, **kw):
        shutter, interlace, scale = kw.pop('shutter', self.shutter), kw.pop('interlace', self.interlace), kw.pop('scale', self.scale)
        depths, window, denoise = kw.pop('depths', self.depths), kw.pop('shutter_window', self.shutter_window), kw.pop('denoise', self.denoise)
        colour, grain, deblock = kw.pop('colour', self.colour), kw.pop('grain', self.grain), kw.pop('deblock', self.deblock)
        dering, deband, lut = kw.pop('dering', self.dering), kw.pop('deband', self.deband), kw.pop('lut', self.lut)
        nlmeans = kw.pop('nlmeans', self.nlmeans)
        return type(self)(*super()._replace(**kw), shutter=shutter, interlace=interlace, scale=scale, depths=depths, shutter_window=window,
                          denoise=denoise, colour=colour, grain=grain, deblock=deblock, dering=dering, deband=deband, lut=lut,
                          nlmeans=nlmeans)

    def __eq__(self, other):
        return (tuple.__eq__(self, other) is True and self.shutter == getattr(other, 'shutter', None)
                and self.interlace == getattr(other, 'interlace', None) and self.scale == getattr(other, 'scale', None)
                and self.depths == getattr(other, 'depths', None) and self.shutter_window == getattr(other, 'shutter_window', None)
                and self.denoise == getattr(other, 'denoise', None) and self.colour == getattr(other, 'colour', None)
                and self.grain == getattr(other, 'grain', None) and self.deblock == getattr(other, 'deblock', None)
                and self.dering == getattr(other, 'dering', None) and self.deband == getattr(other, 'deband', None)
                and self.lut == getattr(other, 'lut', None) and self.nlmeans == getattr(other, 'nlmeans', None))

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        key = (tuple(self), self.shutter) if self.interlace is None else (tuple(self), self.shutter, self.interlace)
        key = key if self.scale is None else key + ('scale', self.scale)
        key = key if self.depths is None else key + ('depths', self.depths)
        key = key if self.shutter_window is None else key + ('shutter_window', self.shutter_window)
        key = key if self.denoise is None else key + ('denoise', self.denoise)
        key = key if self.colour is None else key + ('colour', self.colour)
        key = key if self.grain is None else key + ('grain', self.grain)
        key = key if self.deblock is None else key + ('deblock', self.deblock)
        key = key if self.dering is None else key + ('dering', self.dering)
        key = key if self.deband is None else key + ('deband', self.deband)
        key = key if self.lut is None else key + ('lut', self.lut)
        return hash(key if self.nlmeans is None else key + ('nlmeans', self.nlmeans))

    def __repr__(self):
        return super().__repr__()[:-1] + ', shutter=%r%s%s)' % (self.shutter, ', interlace=%r' % (self.interlace,) if self.interlace is not None else '',
                                                               (', scale=%r' % (self.scale,) if self.scale is not None else '')
                                                               + (', depths=%r' % (self.depths,) if self.depths is not None else '')
                                                               + (', shutter_window=%r' % self.shutter_window if self.shutter_window is not None else '')
                                                               + (', denoise=%r' % (self.denoise,) if self.denoise is not None else '')
                                                               + (', colour=%r' % (self.colour,) if self.colour is not None else '')
                                                               + (', grain=%r' % (self.grain,) if self.grain is not None else '')
                                                               + (', deblock=%r' % (self.deblock,) if self.deblock is not None else '')
                                                               + (', dering=%r' % (self.dering,) if self.dering is not None else '')
                                                               + (', deband=%r' % (self.deband,) if self.deband is not None else '')
                                                               + (', lut=%r' % (self.lut,) if self.lut is not None else '')
                                                               + (', nlmeans=%r' % (self.nlmeans,) if self.nlmeans is not None else ''))

    @classmethod
    def of(cls, yuv):
        """The spec of ``run_clip_u8(yuv=yuv)``; the only place that knows the optional attributes of ``yuv`` and their defaults."""
        dedup, fields = getattr(yuv, 'dedup', None), getattr(yuv, 'fields', None)
        return cls(yuv is not None, getattr(yuv, 'scene_cut', None) is not None, bool(getattr(yuv, 'full_length', False)), int(getattr(yuv, 'depth', 8)),
                   getattr(yuv, 'layout', '420'), tuple(dedup) if dedup is not None else None, fields,
                   getattr(yuv, 'deint_mode', 'bob') if fields is not None else 'bob', shutter=getattr(yuv, 'shutter', None),
                   interlace=getattr(yuv, 'interlace', None), scale=getattr(yuv, 'scale', None), depths=getattr(yuv, 'depths', None),
                   shutter_window=getattr(yuv, 'shutter_window', None), denoise=getattr(yuv, 'denoise', None), colour=getattr(yuv, 'colour', None),
                   grain=getattr(yuv, 'grain', None), deblock=getattr(yuv, 'deblock', None),
                   dering=getattr(yuv, 'dering', None), deband=getattr(yuv, 'deband', None), lut=getattr(yuv, 'lut', None),
                   nlmeans=getattr(yuv, 'nlmeans', None))

    hi = property(lambda self: self.depth > 8, doc='16-bit frames: the samples of a stream above 8 bits')
    reach = property(lambda self: DN.reach(self.denoise[2], self.fields is not None) if self.denoise is not None
                     else 2 if self.fields is not None and self.deint_mode == 'adaptive' else 0,
                     doc='frames before and after a frame that its ingest reads: the adaptive deinterlacer 2 fields, the denoiser R (bobbed fields: 2 R)')

    def _grain_ok(self):
        try:
            return GR.check_params(self.grain) == self.grain
        except ValueError:
            return False

    def check(self, retimed, has_window_index, reuse_frames):
        """Every rule about what goes together, before anything is allocated, for a run on a ``retimed`` runner (built with a ratio)."""
        other, edge_only = self.deint_mode != 'bob', self.hi or self.dedup is not None or self.fields is not None
        deint = deint_conflict(self.deint_mode, self.fields is not None, self.dedup is not None)
        sh, il, sc, dp, win, dn, co = self.shutter, self.interlace, self.scale, self.depths, self.shutter_window, self.denoise, self.colour
        gr, db, dr, bd, lu, nl = self.grain, self.deblock, self.dering, self.deband, self.lut, self.nlmeans
        for bad, what in ((self.fields not in (None, 't', 'b'), "fields must be None, 't' or 'b', got %r" % (self.fields,)),
                          (deint, 'deint_mode %r with fields=%r, dedup=%r' % (self.deint_mode, self.fields, self.dedup)),
                          (edge_only and not self.y4m, '16-bit frames, repeated frames and fields are those of the Y4M edge (yuv=...) only'),
                          (retimed and not self.y4m, 'a retimed runner needs the Y4M edge (yuv=...)'),
                          (other and not reuse_frames, 'deint_mode %r needs reuse_frames (slots are keyed by field)' % (self.deint_mode,)),
                          (self.dedup is not None and not (retimed and has_window_index and reuse_frames),
                           'repeated frames need a retimed runner (r = M for x M), window_index and reuse_frames'),
                          (self.cuts and not (retimed and reuse_frames), 'scene cuts need a retimed runner (r = M for x M) and reuse_frames'),
                          (self.full and not (retimed and has_window_index), 'the full-length timeline needs a retimed runner and window_index'),
                          (sh is not None and not (1 <= sh[0] <= sh[1] and sh[0] <= SH.MAX_SAMPLES),
                           'shutter must be None or (S, D) with 1 <= S <= D and S <= %d, got %r' % (SH.MAX_SAMPLES, sh)),
                          (sh is not None and not (retimed and self.y4m),
                           'a shutter needs the Y4M edge on a retimed runner, built with the fine ratio r D'),
                          (sh is not None and self.dedup is not None,
                           'a shutter does not go with repeated frames (dedup): its groups are laid over the regular fine timeline'),
                          (win is not None and (win not in SH.WINDOWS or sh is None),
                           'shutter_window must be None or one of %s, and only with a shutter, got %r with shutter=%r' % (SH.WINDOWS, win, sh)),
                          (il is not None and not (len(il) == 2 and il[0] in ('t', 'b') and il[1] in IL.LOWPASS),
                           "interlace must be None or (field order 't' / 'b', low-pass mode of %s), got %r" % (IL.LOWPASS, il)),
                          (il is not None and not (retimed and self.y4m), 'interlaced output needs the Y4M edge on a retimed runner'),
                          (sc is not None and not (len(sc) == 3 and sc[0] >= 1 and sc[1] >= 1 and sc[2] in SC.FILTERS),
                           'scale must be None or (w, h, filter of %s), got %r' % (SC.FILTERS, sc)),
                          (sc is not None and not (retimed and self.y4m), 'resized output needs the Y4M edge on a retimed runner'),
                          (dp is not None and not (dp[0] <= dp[1] >= dp[2] and dp[1] == self.depth and all(d in (8, 10, 12, 14, 16) for d in dp[:3])
                                                   and (dp[3] in BD.DITHERS if dp[2] < dp[1] else dp[3] is None)),
                           'depths must be None or (input, working, output depth, dither mode of %s where the output is below the working '
                           'depth, else None) with input <= working == depth >= output, got %r at depth %r' % (BD.DITHERS, dp, self.depth)),
                          (dp is not None and not (retimed and self.y4m), 'a change of bit depth needs the Y4M edge on a retimed runner'),
                          (dn is not None and not (len(dn) == 3 and 0 <= dn[0] <= dn[1] <= 255 and 1 <= dn[2] <= DN.MAX_RADIUS),
                           'denoise must be None or (A, B, R) with 0 <= A <= B <= 255 and 1 <= R <= %d, got %r' % (DN.MAX_RADIUS, dn)),
                          (dn is not None and not (retimed and self.y4m and reuse_frames),
                           'the denoiser needs the Y4M edge on a retimed runner and reuse_frames (slots are keyed by frame)'),
                          (dn is not None and self.dedup is not None,
                           'the denoiser does not go with repeated frames (dedup): kept frames are staged one at a time, without look-ahead'),
                          (dn is not None and other,
                           'the denoiser does not go with deint_mode %r: two deferred look-ahead stages in a row' % (self.deint_mode,)),
                          (co is not None and not (len(co) == 3 and co[0] in (None,) + CL.TRANSFERS and co[1] in (None,) + tuple(CL.y4m.MATRICES)),
                           'colour must be None or (transfer of %s or None, out matrix of %s or None, out full range or None), got %r'
                           % (CL.TRANSFERS, tuple(CL.y4m.MATRICES), co)),
                          (co is not None and not (retimed and self.y4m), 'linear light and an output matrix or range need the Y4M edge on a retimed runner'),
                          (co is not None and co[0] is not None and self.depth > CL.MAX_DEPTH,
                           'linear light needs a working depth of at most %d bits, got %d: above, 16 bits of light do not tell the codes apart'
                           % (CL.MAX_DEPTH, self.depth)),
                          (gr is not None and not self._grain_ok(), 'grain must be None or (S16 in 0..%d, r in 0..2, C16 in 0..16, curve of %s, '
                           'seed in 0..2^32-1), got %r' % (GR.MAX_S16, GR.CURVES, gr)),
                          (gr is not None and not (retimed and self.y4m), 'film grain needs the Y4M edge on a retimed runner'),
                          (db is not None and not (len(db) == 2 and 0 <= db[1] <= db[0] <= 255),
                           'deblock must be None or (A, B) with 0 <= B <= A <= 255, got %r' % (db,)),
                          (db is not None and not (retimed and self.y4m), 'deblocking needs the Y4M edge on a retimed runner'),
                          (dr is not None and not (len(dr) == 3 and 0 <= dr[0] <= 15 and 0 <= dr[1] <= 4 and 3 <= dr[2] <= 6),
                           'dering must be None or (P, S, D) with 0 <= P <= 15, 0 <= S <= 4, 3 <= D <= 6, got %r' % (dr,)),
                          (dr is not None and not (retimed and self.y4m), 'deringing needs the Y4M edge on a retimed runner'),
                          (bd is not None and not (len(bd) == 2 and 0 <= bd[0] <= 8 and 1 <= bd[1] <= 16),
                           'deband must be None or (T, R) with 0 <= T <= 8, 1 <= R <= 16, got %r' % (bd,)),
                          (bd is not None and not (retimed and self.y4m), 'debanding needs the Y4M edge on a retimed runner'),
                          (nl is not None and not (len(nl) == 3 and 0 <= nl[0] <= 16 and 1 <= nl[1] <= 3 and 1 <= nl[2] <= 7),
                           'nlmeans must be None or (S, P, R) with 0 <= S <= 16, 1 <= P <= 3, 1 <= R <= 7, got %r' % (nl,)),
                          (nl is not None and not (retimed and self.y4m), 'spatial denoising needs the Y4M edge on a retimed runner'),
                          (lu is not None and not isinstance(lu, LU.Cube), 'lut must be None or a lut3d.Cube, got %r' % (lu,)),
                          (lu is not None and not (retimed and self.y4m), 'a 3D LUT needs the Y4M edge on a retimed runner'),
                          (lu is not None and self.depth > LU.MAX_DEPTH,
                           'a 3D LUT needs a working depth of at most %d bits, got %d: the gather in front of it keeps its table of at most %d '
                           'entries in LDS' % (LU.MAX_DEPTH, self.depth, 1 << LU.MAX_DEPTH))):
            if bad:
                raise ValueError('WindowRunner.run_clip_u8: ' + what)


def residency_order(extra, wins, near):
    """The order in which a batch makes frames resident, as (position of the window that names it or None, frame index): of the frames ``near``
    (``around`` of the edge) those before the batch's first frame (frames are read in order); ``extra`` (``begin`` of the edge); the frames of the
    windows ``wins``; then the rest of ``near``."""
    first = min(itertools.chain(extra, *wins)) if near else None
    yield from ((None, idx) for idx in near if idx < first)
    yield from ((None, idx) for idx in extra)
    yield from ((wi, idx) for wi, win in enumerate(wins) for idx in win)
    yield from ((None, idx) for idx in near if idx > first)


class FrameSlots:
    """Device ring of input frame slots ``frames`` [n,h,w,3] uint8 (``dtype`` int16: the 16-bit frames of a high-depth Y4M
    stream).  ``slot_of``: frame key -> slot; ``busy[s]``: event of the compute of the batch that last read slot s."""

    def __init__(self, n, h, w, dev, dtype=torch.uint8):
        self.frames = torch.empty((n, h, w, 3), dtype=dtype, device=dev)
        self.reset()

    def reset(self):
        self.slot_of, self.key_of, self.busy, self.next = {}, [None] * len(self.frames), [None] * len(self.frames), 0

    def acquire(self, key, stream):
        """(slot of frame ``key``, must it be uploaded).  A new frame takes the ring's next slot: the frame held there is
        forgotten, and ``stream`` (the one that uploads) waits for the compute that last read it."""
        sl = self.slot_of.get(key)
        if sl is not None:
            return sl, False
        sl = self.next
        self.next = (sl + 1) % len(self.busy)
        if self.key_of[sl] is not None:
            del self.slot_of[self.key_of[sl]]
        if self.busy[sl] is not None:
            stream.wait_event(self.busy[sl])
        self.slot_of[key], self.key_of[sl] = sl, key
        return sl, True

    def release(self, key):
        """Give back the slot of frame ``key``, the one acquired last: the ring's next frame takes it."""
        sl = self.slot_of.pop(key)
        if (sl + 1) % len(self.busy) != self.next:
            raise RuntimeError('FrameSlots.release: frame %r was not the last one acquired' % (key,))
        self.key_of[sl], self.next = None, sl

    def mark_busy(self, read, ev):
        """The slots a batch read (lists of slots) stay busy until ``ev``."""
        for fr in read:
            for sl in fr:
                self.busy[sl] = ev


class Tiler:
    """Device side of a multi-tile plan (``demfi_amd.tiling``).  ``tin`` [nslot, n_tiles, th, tw, 3]: the tiles of every frame
    slot, cropped when the frame is uploaded (``crop``: one ``demfi_u8_tile_crop`` launch per run of consecutive new slots, on the
    upload stream), so a frame is cropped once however many windows read it, and a slot's ``busy`` event covers its tiles too.
    ``stitch``: ONE ``demfi_u8_tile_stitch`` launch pastes the tile outputs of a batch into full frames."""

    def __init__(self, plan, slots, lib, dev, max_frames):
        self.plan, self.nt, self.lib, self.slots = plan, plan.n_tiles, lib, slots
        (self.h, self.w), (self.th, self.tw) = (plan.h, plan.w), plan.tile
        self.rects = np.ascontiguousarray(plan.rects(), dtype=np.int32)
        self.rects_dev = torch.from_numpy(self.rects).to(dev)
        self.tin = torch.empty((len(slots.frames), self.nt, self.th, self.tw, 3), dtype=torch.uint8, device=dev)
        self.offs = torch.empty(max_frames * (self.nt + 1), dtype=torch.int64, device=dev)    # reused in stream order

    def crop(self, sls, stream):
        fr = self.slots.frames
        for s0, cnt in consecutive(sls):
            L.check(self.lib.demfi_u8_tile_crop(fr[s0].data_ptr(), fr.stride(0), self.tin[s0].data_ptr(), cnt, self.h, self.w, self.th,
                                                self.tw, self.nt, self.rects.ctypes.data, self.rects_dev.data_ptr(), stream.cuda_stream),
                    'u8_tile_crop')

    def stitch(self, src, src_offs, dst, dst_offs, stream):
        """Frame f = the tiles at src + src_offs[f, j] -> the frame at dst + dst_offs[f] (numpy int64 byte offsets)."""
        n = len(dst_offs)
        if n == 0:
            return
        od = self.offs[:n * (self.nt + 1)]
        od.copy_(torch.from_numpy(np.concatenate([np.asarray(src_offs, np.int64).reshape(-1), np.asarray(dst_offs, np.int64)])).pin_memory(),
                 non_blocking=True)
        L.check(self.lib.demfi_u8_tile_stitch(src.data_ptr(), od.data_ptr(), dst.data_ptr(), od[n * self.nt:].data_ptr(), n, self.h, self.w,
                                              self.th, self.tw, self.nt, self.rects.ctypes.data, self.rects_dev.data_ptr(),
                                              stream.cuda_stream), 'u8_tile_stitch')


class BgrEdge:
    """uint8 BGR [h,w,3] frames in; sink(k, St [M-1,h,w,3], S0S1 [2,h,w,3]) out (views of pinned staging buffers).  Tiled: window w
    is the n_tiles runs w * n_tiles + j into ``tout`` / ``ts01``; out and s01 are then halves of one buffer (one stitch launch)."""

    def __init__(self, runner, batch, slots, tiler=None):
        self.rn, self.slots, self.tiler = runner, slots, tiler
        self.fh, self.fw = (tiler.h, tiler.w) if tiler else (runner.h, runner.w)
        dev, shape, m1 = runner.engine.device, (self.fh, self.fw, 3), runner.mfi - 1
        if tiler:
            def halves(n, sh):                       # [n, M-1] + sh and [n, 2] + sh in one allocation
                buf, cut = torch.empty((n * (m1 + 2),) + sh, dtype=torch.uint8, device=dev), n * m1
                return buf, buf[:cut].view((n, m1) + sh), buf[cut:].view((n, 2) + sh)
            self.buf, self.out, self.s01 = zip(*[halves(batch, shape) for _ in range(2)])
            self.tbuf, self.tout, self.ts01 = halves(batch * tiler.nt, (tiler.th, tiler.tw, 3))
            self._stitch_offs = {}
        else:
            self.out = [torch.empty((batch, m1) + shape, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.s01 = [torch.empty((batch, 2) + shape, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.h_out = [torch.empty((batch, runner.mfi - 1) + shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.h_s01 = [torch.empty((batch, 2) + shape, dtype=torch.uint8).pin_memory() for _ in range(2)]

    def begin(self, yuv, window_index, first_win):
        return ()

    attach = around = lambda self, *args: []         # noqa: E731  nothing to attach to; no frame needed besides a batch's own
    flush = lambda self, *args: None                 # noqa: E731  nothing is held back past the last batch

    def upload(self, sl, idx, f):
        if tuple(f.shape) != (self.fh, self.fw, 3) or f.dtype != torch.uint8:
            raise ValueError('frame %d: expected uint8 [%d,%d,3], got %s %s' % (idx, self.fh, self.fw, f.dtype, tuple(f.shape)))
        self.slots.frames[sl].copy_(f, non_blocking=True)

    def uploaded(self, new, h2d):
        if self.tiler:
            self.tiler.crop([sl for _, sl in new], h2d)

    def run(self, i, n, wins, frames, cur):
        cnt, tl = len(wins), self.tiler
        if not tl:
            self.rn.run_windows_u8([[self.slots.frames[sl] for sl in fr] for fr in frames], out=self.out[i][:cnt], s01=self.s01[i][:cnt])
            return cnt, frames
        nt = tl.nt
        self.rn.run_windows_u8([[tl.tin[sl, j] for sl in fr] for fr in frames for j in range(nt)], out=self.tout[:cnt * nt],
                               s01=self.ts01[:cnt * nt])
        offs = self._stitch_offs.get(cnt)
        if offs is None:                             # frame (w, p) of out, then of s01: its tiles are rows w * nt + j of tout / ts01
            m1, fsz, tsz = self.rn.mfi - 1, self.out[i][0, 0].numel(), self.tout[0, 0].numel()
            w, j = np.arange(cnt, dtype=np.int64)[:, None, None], np.arange(nt, dtype=np.int64)[None, None, :]
            src, dst = [], []
            for k, d0, s0 in ((m1, 0, 0), (2, self.out[i].numel(), self.tout.numel())):
                p = np.arange(k, dtype=np.int64)[None, :, None]
                src.append((s0 + ((w * nt + j) * k + p) * tsz).reshape(-1, nt))
                dst.append((d0 + (w * k + p) * fsz)[:, :, 0].reshape(-1))
            offs = self._stitch_offs[cnt] = (np.concatenate(src), np.concatenate(dst))
        tl.stitch(self.tbuf, offs[0], self.buf[i], offs[1], cur)
        return cnt, frames

    def d2h(self, i, cnt):
        self.h_out[i][:cnt].copy_(self.out[i][:cnt], non_blocking=True)
        self.h_s01[i][:cnt].copy_(self.s01[i][:cnt], non_blocking=True)

    def drain(self, i, k0, cnt, sink):
        for j in range(cnt):
            sink(k0 + j, self.h_out[i][j], self.h_s01[i][j])


class KeptFrames:
    """``host_frames`` and ``windows`` of a --dedup run: the kept frames of an input (``y4m.Frames`` ``raw``), indexed by kept
    index.  Pulling ``windows()`` reads the input: every frame is staged in a device slot and scored there against the last
    kept frame (``y4m_edge.DedupProbe``: ``stage`` / ``block_counts``), a repeat's slot is recycled at once, and window k is handed out when
    ``cadence.ready`` says it can be planned -- B2 or the end of the input is known.  So the pipeline finds every frame a
    window names already resident, and only kept frames occupy slots.  ``det``: the ``cadence.Detector``; ``s`` its kept
    times, ``n`` the input's length once its end was seen, ``first_window`` the first window handed out, ``st_frames`` the St
    frames planned."""

    def __init__(self, raw, det, r, full_length=False):
        self.raw, self.det, self.r, self.full = raw, det, Fraction(r), bool(full_length)
        self.s, self.n, self.first_window, self.edge, self.ref, self.st_frames = det.kept, None, None, None, None, 0

    def __getitem__(self, j):
        raise IndexError('kept frame %d is not resident: --dedup stages every frame before a window names it' % j)

    def index(self, j):
        """Window index of the j-th window handed out."""
        return self.first_window + j

    def _probe(self):
        """Examines the next input frame; False at the end of the input."""
        det, i = self.det, self.det.next
        if not self.raw.has(i):
            self.n = i
            return False
        key = len(det.kept)
        sl = self.edge.stage(key, i, self.raw[i])
        if det.push(i, None if det.forced() else self.edge.block_counts(sl, self.ref)):
            self.ref = sl
            self.edge.keep(key, sl)
        else:
            self.edge.discard(key)
        return True

    def _know(self, k):
        """Reads on until window k can be planned."""
        while self.n is None:
            if len(self.s) > k + 2 and not self.full:
                self.raw.has(self.s[k + 2] + 2)      # read ahead only: is tau = s_{k+2} the last output?
            if K.ready(k, self.s, self.raw.next, None, self.full) or not self._probe():
                return

    def windows(self):
        """(B0, B1, B-1, B2), kept indices clamped at the ends of the kept sequence, of every window in order."""
        while self.n is None and len(self.s) < 2:
            self._probe()
        if not self.s:
            return
        if len(self.s) == 1:                         # the end was seen: one kept frame, held
            if R.n_output_frames(self.n, self.r, self.full) > 0:
                self.first_window = -2
                yield (0, 0, 0, 0)
            return
        k = -1
        while True:
            self._know(k)
            if self.n is not None and k + 2 > len(self.s) - 1:
                return
            if K.window_outputs(k, self.r, self.s, self.n, self.full):
                if self.first_window is None:
                    self.first_window = k
                yield S.runner_order(K.window_tuple(k, self.s, self.n))
            elif self.first_window is not None:
                return                               # past the last output
            k += 1


class ClipPipeline:
    """The batch loop of ``WindowRunner.run_clip_u8`` for one batch size and one ``EdgeSpec`` (``key``; both size the buffers): H2D of a batch's new
    frames, its compute, the drain of the previous batch and its D2H, on three streams over two sets of output buffers."""

    def __init__(self, runner, batch, spec):
        dev = self.dev = runner.engine.device
        runner = weakref.proxy(runner)               # the runner owns this pipeline: no reference cycle keeps its buffers alive
        self.batch, self.key = batch, (batch, spec)
        self.h2d, self.d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        plan = runner.tiles
        fh, fw = (plan.h, plan.w) if plan is not None else (runner.h, runner.w)
        look = 2 * spec.reach                        # the frames an ingest stage reads behind a batch's frames and ahead of them (adaptive: two fields each)
        self.slots = FrameSlots(max(2 * batch + 8 + look, 8 * batch), fh, fw, dev, torch.int16 if spec.hi else torch.uint8)
        # 16-bit frames: tiles are read and written inside the full frames.  8-bit: the frames stitched per batch are a run's J + 2
        # (a cut window is two runs), or M + 1
        per_window = max_runs(runner.ratio, spec.cuts, spec.dedup) * (R.max_instants(runner.ratio) + 2) if spec.y4m else runner.mfi + 1
        tiler = None if plan is None else TileGrid(plan) if spec.hi else Tiler(plan, self.slots, runner.lib, dev, batch * per_window)
        self.edge = Y4mEdge(runner, batch, self.slots, spec, tiler, self.h2d) if spec.y4m else BgrEdge(runner, batch, self.slots, tiler)

    def run(self, host_frames, windows, sink, reuse_frames, yuv, window_index):
        edge, slots, h2d, cur = self.edge, self.slots, self.h2d, torch.cuda.current_stream(self.dev)
        slots.reset()
        edge.attach(host_frames, yuv)
        it = iter(windows)
        wins = list(itertools.islice(it, self.batch))
        if not wins:
            return 0
        extra = edge.begin(yuv, window_index, wins[0])
        has = getattr(host_frames, 'has', lambda i: 0 <= i < len(host_frames))
        ev_d2h = [None, None]             # D2H of the batch that last wrote output buffer i
        pending = None                    # (buffer, first window, what edge.run returned) of the batch whose D2H is in flight
        n = b = 0
        while wins:
            i = b & 1
            # ---- H2D of the frames this batch needs (copy stream) -------------------------------------------------
            new = []                      # (frame, slot) uploaded for this batch
            frames = [[] for _ in wins]   # the slots of every window's frames
            with torch.cuda.stream(h2d):
                for wi, idx in residency_order(extra, wins, edge.around(itertools.chain(extra, *wins), has)):
                    sl, fresh = slots.acquire(idx if reuse_frames or wi is None else (b, wi, idx), h2d)
                    if fresh:
                        edge.upload(sl, idx, host_frames[idx])
                        new.append((idx, sl))
                    if wi is not None:
                        frames[wi].append(sl)
                edge.uploaded(new, h2d)
                ev_up = torch.cuda.Event()
                ev_up.record(h2d)
            # ---- compute (pipelined windows) ---------------------------------------------------------------------
            cur.wait_event(ev_up)
            if ev_d2h[i] is not None:
                cur.wait_event(ev_d2h[i])                     # the D2H of batch b-2 has read this output buffer
            res, read = edge.run(i, n, wins, frames, cur)
            ev = torch.cuda.Event()
            ev.record(cur)
            slots.mark_busy(read, ev)
            # ---- hand the previous batch to the sink while this one computes ------------------------------------------
            if pending is not None:
                self._drain(pending, ev_d2h, sink)
            # ---- D2H of this batch (copy stream), into pinned staging ------------------------------------------------
            with torch.cuda.stream(self.d2h):
                self.d2h.wait_event(ev)
                edge.d2h(i, res)
                ev_d2h[i] = torch.cuda.Event()
                ev_d2h[i].record(self.d2h)
            pending = (i, n, res)
            n, b, extra = n + len(wins), b + 1, ()
            wins = list(itertools.islice(it, self.batch))
        self._drain(pending, ev_d2h, sink)
        res = edge.flush(b & 1, cur)                 # what the edge held back past the last batch: it counts to the last window
        if res is not None:                          # buffer set b & 1 is free: the batch that last used it was drained
            ev = torch.cuda.Event()
            ev.record(cur)
            with torch.cuda.stream(self.d2h):
                self.d2h.wait_event(ev)
                edge.d2h(b & 1, res)
                ev_d2h[b & 1] = torch.cuda.Event()
                ev_d2h[b & 1].record(self.d2h)
            self._drain((b & 1, n - 1, res), ev_d2h, sink)
        return n

    def _drain(self, pending, ev_d2h, sink):
        i, k0, res = pending
        ev_d2h[i].synchronize()
        if sink is not None:
            self.edge.drain(i, k0, res, sink)
