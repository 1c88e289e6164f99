"""Video streams in, video streams out: x M interpolation of a YUV4MPEG2 (Y4M) stream, or retiming to any other frame rate.

    ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe - | python -m demfi_amd.video - - --mfi 8 | ffmpeg -f yuv4mpegpipe -i - out.mp4
    ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe - | python -m demfi_amd.video - - --fps 60000/1001 | ffmpeg -f yuv4mpegpipe -i - out.mp4

The frames are those of the folder path (``python -m demfi_amd.clip``) for the same pixels, in the order of the reference's
``test_custom`` folder sorted by name (``clip.output_names`` / ``clip.deblurred_writes``): per window k, S0 (deblurred B0) and
then St for t = 1/M .. (M-1)/M; after the last window its S1.  n input frames give (n-3)*M + 1 output frames: the first and
the last input frame have no output of their own, as in the reference.  ``--fps F_out`` (an exact fraction, F_out >= F_in) puts
output frame i at input time 1 + i * F_in / F_out instead and runs only the time instants those frames need
(``demfi_amd.retime``); ``--fps M*F_in`` gives the bytes of ``--mfi M``.  ``--downconvert`` lets F_out lie below F_in, down to 1/64 of
it (60p -> 25p; behind ``--deinterlace`` below the field rate, so that ``--deinterlace --downconvert --fps 50 --interlace tff`` is
59.94i -> 50i, header ``F25:1 It``; behind ``--ivtc`` below the film rate): the same timeline with the output frames further apart.
Window k owns the outputs ceil(k r) .. ceil((k+1) r) - 1, possibly none; a window that owns none runs no instant and launches nothing
of the network (``last_windows_skipped``), though its frames are uploaded as ever, once each, for the scene scores.  Every switch below
works with it except ``--dedup``, which is refused once the header is known; with F_out >= F_in it changes nothing.  Each written frame
then stands for more than one input frame period, so ``--shutter`` belongs with it.  ``--full-length`` covers the input's whole timeline
instead: output frame i sits at input time i * F_in / F_out, so n frames give n*M (ceil(n * F_out / F_in)) output frames that
stay aligned with the input's audio; the clip's ends clamp the windows next to them like scene cuts and the last input frame
is held to the end.

The colour conversion runs on the GPU next to the uint8 ingest / sink (csrc/yuv.hip, defined by ``y4m.yuv420_to_bgr_np`` /
``y4m.bgr_to_yuv420_np``): 4:2:0 payloads go host -> HBM (half the bytes of BGR), are converted once per frame into the
runner's BGR frame slots, and every computed batch is gathered back into a stream-order device buffer in one launch
(``WindowRunner.run_clip_u8(yuv=...)``).  There is one path for all rates: every window runs the plan ``demfi_amd.retime`` gives
it for r = F_out / F_in, and ``--mfi M`` is r = M.  One rank reads a stream (stdin included) in bounded batches and writes each batch
as it drains; under ``torch.distributed.run`` every rank takes ``dist.shard_windows``' block of a regular file and writes its
frames at their byte offsets of the output file (no collective on the data path).

``--high-depth`` also takes 10-, 12-, 14- and 16-bit 4:2:0 (C420p10 .. C420p16: 16-bit little-endian samples, what
``ffmpeg -pix_fmt yuv420p10le -strict -1 -f yuv4mpegpipe`` writes) and gives the output at the input's depth: the same path on
16-bit frames (csrc/yuv_family.hip, ``y4m.yuv420_to_bgr16_np`` / ``y4m.bgr16_to_yuv420_np``) from the payload to the network's input and
from its fp32 output frames back; only the fused uint8 store of the fp16 engine is replaced by one egress kernel per frame.
With ``--dtype fp16`` the network's input record and features are fp16, which resolves 10-bit video fully and about 12 bits at
best near the ends of the range; ``--dtype fp32`` carries all 16 bits.  ``--tile-high-depth`` lets such a stream run as tiles
(``--tile``): the 16-bit ingest and egress kernels address every tile inside the full frames (csrc/frames16.hip), so no tile is
copied out of a frame or pasted back into one.

``--any-layout`` also takes 4:2:2, 4:4:4 and grey streams (C422, C444, Cmono, what ``ffmpeg -pix_fmt yuv422p / yuv444p / gray -f
yuv4mpegpipe`` writes; together with ``--high-depth`` their 10- to 16-bit forms C422pNN, C444pNN, CmonoNN) and gives the output in
the input's layout and depth.  Only the two conversions at the edge know the layout (csrc/yuv_family.hip, ``y4m.yuv_to_bgr_np`` /
``y4m.bgr_to_yuv_np`` and their 16-bit forms): the payload of P samples becomes the same BGR frame slots, and retiming, scene cuts
(scored over the payload's P samples), the full-length timeline, tiles (deep layouts with ``--tile-high-depth``) and rank sharding run
as they do for 4:2:0.

``--deinterlace`` also takes interlaced streams (``It``: top field first, ``Ib``: bottom field first; what ``ffmpeg -f yuv4mpegpipe``
writes for 1080i, 576i, 480i and DV material) and bobs them: every payload gives two progressive frames, one per field in field
order, each at its own time instant, so n payloads at F are a progressive stream of 2n frames at 2F ("50i in, 100p out" with
``--mfi 2``).  The payload is uploaded as it is and one launch rebuilds the other field's rows in place by an edge-directed line
average (csrc/deint.hip, defined by ``deint.bob_plane_np``) before it is converted; everything behind that -- rates, scene cuts,
repeated frames, the full-length timeline, tiles, depths, layouts, rank sharding -- runs on the progressive stream unchanged.
``--fps`` and ``--mfi`` count from the field rate 2F.  The output is progressive unless ``--interlace`` (below) weaves it back into fields.  Not offered: mixed-mode streams (``Im``;
film carried by pulldown goes through ``--ivtc`` below); the quarter-row chroma offset of interlaced 4:2:0 fields is not modelled; a
payload is uploaded once per field.

``--deinterlace-mode adaptive`` (with ``--deinterlace``; the default ``bob`` is the above) rebuilds the missing rows motion-adaptively
instead: the bob's value is clamped to an interval around the average of the fields before and after, whose width is yadif's
temporal difference over fields f-2 .. f+2 with its spatial check (csrc/deint.hip ``demfi_yuv_deint_adaptive``, defined by
``deint.adaptive_plane_np``).  Static parts of the picture keep their full vertical resolution and stop flickering at the field
rate, so the network is not shown motion that is not there; moving parts and scene cuts fall back to the bob's value.  Field f
is rebuilt once fields f+1 and f+2 are uploaded (two fields of lookahead; a rank's block also reads the two fields before it and
after it), in place and without uploading any payload more often; an output field depends on payloads p-1, p and p+1 of the
input only, whatever the batch size and the rank count.  Works with every switch above except ``--dedup``, which stages and
discards fields one at a time: the two together are refused, ``--deinterlace-mode bob`` is the way out.

``--ivtc`` takes film carried by 3:2 pulldown (24p as 29.97 frames/s: NTSC DVDs, broadcast captures; flagged ``It``, ``Ib``, ``Im`` or,
wrongly, ``Ip``) and undoes the pulldown in front of everything else, as ffmpeg's ``fieldmatch,decimate`` does
(``demfi_amd.telecine``): every payload keeps its top field and takes the bottom field of itself, the payload before or the one
after, whichever weaves to the least combed frame, and of every five matched frames the one that repeats its predecessor most
closely is dropped.  n payloads at F are a progressive stream of n - floor(n/5) frames at 4F/5, so ``--ivtc --fps 60000/1001`` is
the true 23.976 -> 59.94; ``--fps`` and ``--mfi`` count from the film rate.  The comb scores of the three candidates of five
payloads are ONE launch and the decimation metrics another (csrc/ivtc.hip, defined by ``telecine.comb_counts_np`` /
``woven_sad_np``) over a small device ring of luma planes on a stream of its own; the kept frames are woven on the host.  A matched
frame that is still combed (more than ``--ivtc-combpel`` samples in a 16x16 block) is bobbed from its top field
(``--ivtc-combed bob``, the default) or passed through (``keep``) and reported.  Not offered: hybrid film / video material (30i
sections are decimated like the rest), other cadences, a scene-change guard for the decimator, more than one
rank, and ``--ivtc`` together with ``--deinterlace``.  Interlaced output is ``--interlace`` below.

``--crop auto`` finds letterbox and pillarbox bars (scope films in 16:9, 4:3 in 16:9, windowboxed captures) and keeps them away from
the network (``demfi_amd.letterbox``): a pre-pass counts, for every row and column of the luma plane of the probed payloads
(``--crop-probe``, default all), the samples above ``--crop-limit`` (24 at 8 bits, ffmpeg ``cropdetect``'s) in ONE launch per 16
planes (csrc/crop.hip, defined by ``letterbox.line_counts_np``); a line with more than ``--crop-noise`` (1/256) of its samples lit is
picture, the union of the frames' extents, grown to the chroma grid, is the picture rectangle.  Every payload is then cropped on the
host as the last stage in front of the frames (behind ``--ivtc``'s film frames, in front of the deinterlacer, whose row pairs the
alignment keeps), everything downstream -- the network, scene cuts, repeated frames, tiles, rank sharding -- runs on the smaller
frame, and every output payload is padded back with exact black of the stream's range (``--crop-output pad``, the default: the
output has the input's size) or written as it is (``cropped``).  The forward's cost follows the area, so 1920x800 of picture in
1920x1080 runs about a quarter faster, and no interpolated frame carries picture into the bars.  ``--crop T:B:L:R`` gives the four
bar widths instead: nothing is probed, and it works on pipes, where ``auto`` is refused because the bars of a stream are known only
at its end.  With several ranks every rank runs the same pre-pass and arrives at the same rectangle.  A rectangle below 64x64 is
not cropped to (``auto``: reported; explicit: an error, like a misaligned one); ``auto`` on a clip without bars, or an all-black
one, gives the bytes of a run without the switch.  Not offered: bars that change within a stream (the union is taken), ``--crop`` on
``demfi_amd.clip``, restoring the input's own bar samples (output bars are exact black); scene-cut and repeated-frame decisions are
made over the cropped payloads, so they can differ from those of an uncropped run.

``--shutter ANGLE`` (degrees, N or N/D, 0 < ANGLE <= 360) with ``--shutter-samples S`` (1 .. 32, default 4) synthesizes motion blur
(``demfi_amd.shutter``): every written frame is the average of S finer frames spread over an exposure of ANGLE/360 of its frame period,
from its own time on, instead of one sharp frame -- 180 degrees is the film look, and 24 -> 60 stops strobing.  D = 360 S / ANGLE must
be an integer; the fine stream is this module's own timeline at the ratio r D (at most ``retime.MAX_RATIO``, checked once the header is
known), written frame c averages the fine frames c D .. c D + S - 1 that exist and lie in the scene of the first (``--scene-cut``), and
the written stream has the header, the length and the timing of a run without the switch.  The runner is built for the fine ratio and
``shutter.filter_plan`` leaves every window only the instants its samples need; behind the batch's gather ONE launch
(csrc/shutter.hip ``demfi_payload_mix``, defined by ``shutter.mix_np``: (2 sum + k) // (2 k) of the stored samples, round half up, the
payload one flat array) mixes every group whose last sample has arrived into the buffer that crosses D2H, and the samples of the group
still open carry over to the next batch on the device, so the bytes do not depend on the batch size.  ``--shutter-window box|triangle``
(default ``box``; an error without ``--shutter``) weighs the samples: triangle gives sample j the weight min(j + 1, S - j), and a group
mixes to (2 sum w x + W) // (2 W) with W the sum of the weights it keeps (csrc/shutter.hip ``demfi_payload_mix_w``, defined by
``shutter.mix_np(..., weights=...)``; ONE launch as for the box).  With ``--downconvert`` the fine ratio r D may lie below D and below 1:
a window then brings fewer than D fine frames, or none.  Works with every switch above
(the stage sits behind whole payloads; run behind each of them on the GPU except ``--tile-high-depth``, whose two halves are) except
``--dedup``; one rank.  Not offered: linear-light mixing (the average is taken over the
gamma-encoded samples), gaussian or free weights, an exposure centred on the frame time, ``--dedup`` (also with ``--downconvert`` alone
below the input rate), several ranks, ``demfi_amd.clip``.  Without the switch no buffer, launch or stream is added and every byte stays
the same.

``--interlace tff|bff`` with ``--interlace-lowpass off|linear|complex`` (default ``linear``) writes interlaced output
(``demfi_amd.interlace``): frames 2q and 2q + 1 of the progressive stream a run without the switch writes (with ``--shutter``: its mixed
frames) become the first and the second field in time of written payload q -- rows of parity ``deint.field_parity(order, 0)`` of every
plane from the first, the others from the second --, an odd last frame is woven with itself, and the header is the progressive one with
``It`` / ``Ib`` and half the rate.  ``--fps`` and ``--mfi`` keep their meaning: they name the field rate, as behind ``--deinterlace``, so
``--deinterlace --fps 60000/1001 --interlace tff`` is 50i -> 59.94i (header ``F30000:1001 It``), and 25p or ``--ivtc`` film go to 59.94i
the same way.  The low-pass damps interline twitter; it is computed from rows of the one frame that owns the output row.  Behind the
gather (behind the mix with ``--shutter``) ONE launch per batch (csrc/interlace.hip ``demfi_payload_weave``, defined by
``interlace.weave_payload_np``) weaves every pair whose second frame has arrived into the buffer that crosses D2H, half the bytes of the
progressive run; the one open frame carries over to the next batch on the device, so the bytes do not depend on the batch size.  Works
with every switch above; a payload may hold fields of two scenes, which is ordinary interlaced video.  With ``--crop`` the bars go back
on the host behind the weave, and the rectangle must keep field parity in every plane: rows in units of 2, of 4 for 4:2:0 (``auto`` grows
to that grid, an explicit misaligned rectangle is the usual error).  One rank.  Not offered: the quarter-row chroma offset of
interlaced 4:2:0 fields, fusing the weave into the gather so that unused rows are never converted, ``Im`` output, several ranks,
``demfi_amd.clip``, numeric equality with ffmpeg's ``interlace`` / ``tinterlace`` filters.  Without the switch no buffer, launch or stream
is added and every byte stays the same.

``--scale WxH`` (width first, as ffmpeg's ``-s``) with ``--scale-filter lanczos3|bicubic|bilinear`` (default ``lanczos3``) resizes the
output on the GPU (``demfi_amd.scale``), the other half of a standards conversion: 576i50 -> 480i59.94 is ``--deinterlace --fps 60000/1001
--scale 720x480 --interlace tff``.  Every progressive payload a run without the switch writes (with ``--shutter``: its mixed frames) is
resampled plane by plane with a separable polyphase filter in exact integers (Q14 weights that sum to one, six fractional bits between the
passes): behind the gather and the mix, in front of the weave, so the scaler never sees woven fields.  ONE launch per batch
(csrc/scale.hip ``demfi_payload_scale``, defined by ``scale.scale_payload_np``; the weights come from the tables of ``scale.axis_table``
alone) writes the buffer that crosses D2H or that the weave reads; only resized payloads leave the device.  The header gets W, H and
the pixel aspect that keeps the display aspect (720x576 ``A16:15`` -> 720x480 ``A8:9``).  The stage keeps nothing from one payload to the
next, so it works with every switch above and with several ranks (as far as the other switches do).  With ``--crop`` only under
``--crop-output cropped``: the picture rectangle is what is scaled (``pad`` is refused); with ``--interlace`` H lies on the interlaced
grid (rows in units of 2, of 4 for 4:2:0).  A shrink is limited to 32 taps an axis (16:3 with lanczos3, 8:1 bicubic, 16:1 bilinear).  A
size equal to the run's own builds no stage and gives the bytes of a run without the switch.  Not offered: scaling in front of the
network (cheaper for a shrink), chroma siting offsets (chroma planes are resampled centre-aligned, as planes in their own right),
``-1`` / keep-aspect sizes, ``demfi_amd.clip``, numeric equality with swscale or zimg (linear-light resampling: ``--linear-light``).  Without the switch no
buffer, launch or stream is added and every byte stays the same.

``--work-depth W`` and ``--out-depth D`` (8, 10, 12, 14 or 16 each) with ``--dither bayer|none`` (default ``bayer``) choose the stream's bit
depth (``demfi_amd.bitdepth``).  work = W if given, else max(input depth, D); out = D if given, else the INPUT's depth: ``--out-depth 10``
turns an 8-bit stream into ``C420p10`` for a Main10 encoder, ``--work-depth 12`` alone is 8 -> 12 -> 8, dithered.  With a working depth above
the input's every payload is uploaded at the input's sample size and promoted on the GPU right behind its copy (csrc/bitdepth.hip
``demfi_payload_promote``, one launch per run of uploaded slots), so everything downstream -- the deinterlacer, scene scores, the repeated-frame
probe, the 16-bit frame path, the network's egress, the shutter's mix, the scaler, the weave -- sees and rounds a W-bit stream.  With an
output depth below the working depth every written payload is requantised as the last device stage, gather -> mix -> scale -> weave ->
requant -> D2H (``demfi_payload_requant``, one launch per batch), so only D-bit payloads leave the device: 16 -> 8 sends half the bytes.  One
integer rule, out = clip(off_out + floor(((v - off_in) num + T) / den), 0, peak_out) (``bitdepth.convert_payload_np``): limited range is a
pure shift in every plane, full range scales by peak_out / peak_in around 0 (luma) and 2^(d-1) (chroma); T = den / 2 going up and with
``none``, with ``bayer`` going down the threshold of the 8x8 ordered-dither index of the sample's position in its plane, the same in every
frame, and with ``--interlace`` taken from the row within its field.  An input above 8 bits still needs ``--high-depth``, which says what is
taken; an 8-bit input with a deeper working depth runs on the 16-bit frame path without it; with ``--tile`` a working depth above 8 needs
``--tile-high-depth``.  ``--dtype fp16`` resolves 10 bits fully and about 12 at best, so W >= 12 wants ``--dtype fp32``; it is not refused.
``--ivtc`` and ``--crop auto`` decide in front of the device stages on the input's own samples, at the input's depth.  Both stages keep
nothing between payloads: every switch above and several ranks work.  Refused: W below the input's depth, D above W, ``--dither`` where
nothing is requantised.  Depths that resolve to the input's build no stage, no buffer and no launch and give the bytes of a run without the
switches.  Not offered: error diffusion, random or blue-noise dither, patterns that change from frame to frame, ``demfi_amd.clip`` (changing
the range or the matrix on the way: ``--out-matrix`` / ``--out-range``).

``--linear-light [bt709|srgb]``, ``--out-matrix auto|bt601|bt709`` and ``--out-range limited|full`` (``demfi_amd.colour``): with
``--linear-light`` the shutter's mix and the scaler work on light, not on the stored, gamma-encoded samples: the gather writes linear
payloads (uint16 planes B, G, R through the inverse OETF's table), the unchanged mix and scale kernels run on those, and an encode stage
takes them back, gather-to-linear -> mix -> scale -> encode -> weave -> requant (csrc/colour.hip ``demfi_bgr_to_linear_gather`` /
``demfi_linear_to_yuv``, defined by ``colour.linearize_np`` / ``colour.encode_payload_np``).  Working depths 8, 10 and 12 (above: refused
once the header is known); without ``--shutter`` or an effective ``--scale`` it builds nothing.  ``--out-matrix`` / ``--out-range`` bind the
gather (or the encode) to another matrix and range than the input's; ``auto`` is BT.709 when the height written is 720 or more; the
requantisation, the black of ``--crop-output pad`` and the header's XCOLORRANGE follow the range written, everything in front of the network
keeps the input's.  Not offered: primaries / gamut conversion, PQ and HLG, linear-light ``--interlace-lowpass`` or ``--denoise``, a matrix
tag (Y4M has none), ``demfi_amd.clip``.  Without the three switches no buffer, table, launch or stream is added and every byte stays the same.

``--denoise [A[:B]]`` with ``--denoise-radius R`` (1 .. 3, default 2) cleans noisy input in front of the network (``demfi_amd.denoise``): a
deblurring network sharpens grain and tape noise with everything else, and noise that differs from frame to frame is motion that is not
there -- it hurts the flow and inflates the scene scores.  Every stored sample becomes the rounded mean of itself and of the samples at its
position in up to R frames before and R after: each side walks outward on its own and stops for good at the first sample that differs from
the frame's own by more than A or brings the side's accumulated difference above B (8-bit steps, 0 <= A <= B <= 255, default 5:10, A alone
is A:2A, one pair for every plane, shifted to the working depth), the idea of ffmpeg's ``atadenoise`` in its serial mode; ``--denoise 0`` is
the identity.  The stage sits at the ingest, H2D -> promote (``--work-depth``) -> bob -> denoise -> everything else: ONE launch per batch
(csrc/denoise.hip ``demfi_payload_denoise``, defined by ``denoise.denoise_payload_np``; the payload one flat array, so every depth and layout
is served) writes the denoised payloads into a second buffer beside the uploaded ones, which the denoiser alone reads from then on; the
conversion to frames, the tiles and the scene scores read the denoised ones, so a run with the switch writes the bytes of a run without it
over the stream denoised on the host.  Behind ``--deinterlace`` (bob) frame f is field f and its neighbours are the fields of the same
parity f +- 2, f +- 4, ..  A frame is denoised once the R frames (2 R fields) after it are uploaded, in the batch that first names it; a
rank's block also reads that many frames before it and after it; no payload is uploaded more often, and an output frame depends on the
input frames f - R .. f + R only, whatever the batch size and the rank count.  ``--ivtc`` and ``--crop`` are host stages in front: their
frames are ordinary frames, and they decide on the input's own samples.  Works with every switch above except ``--dedup`` (kept frames are
staged one at a time, without look-ahead) and ``--deinterlace-mode adaptive`` (two deferred look-ahead stages in a row), both refused
before anything is allocated.  Not offered: spatial filtering in this stage (``--nlmeans`` is that stage), separate chroma thresholds, motion-compensated averaging, stopping at
detected cuts (the thresholds do that per sample), numeric equality with ffmpeg's ``atadenoise``, decisions of ``--ivtc`` / ``--crop auto`` on
denoised samples, ``demfi_amd.clip``.  Without the switch no buffer, table, launch or slot is added and every byte stays the same.

``--grain S`` with ``--grain-size 0|1|2``, ``--grain-chroma C``, ``--grain-curve film|flat`` and ``--grain-seed N`` adds synthetic film grain to
every progressive payload the run would hand to the weave, the requantiser or D2H (``demfi_amd.grain``): ``--denoise`` removes grain on
purpose, the network, ``--shutter`` and ``--scale`` smooth what is left, and the result looks synthetic next to untouched material and bands
at 8 and 10 bits.  S is the grain's standard deviation in 8-bit code values at the curve's peak (0 .. 8, in sixteenths), the size how coarse
it is (binomial taps over white cells; default 1), C the chroma strength relative to luma (0 .. 1, default 0.5; 0: luma only), the curve
``film`` (default: peaks in the midtones, a quarter at black and white, by the frame's own luma) or ``flat``, the seed a uint32 (default 0).
The chain is gather -> mix -> scale -> encode -> grain -> weave -> requant -> D2H: ONE launch per batch (csrc/grain.hip
``demfi_payload_grain``, byte for byte ``grain.grain_payload_np``) behind everything that would average grain away and in front of the weave
(both fields of a payload get independent grain) and the dither.  The rule: out = clip(v + ((F G[luma code] + 2^15) >> 16), min(lo, v),
max(hi, v)) with F a hashed, binomially filtered field of (seed, frame, plane, x, y) and G a host-built gain table; grain never pushes a
legal sample out of the legal range and never pulls an illegal one in.  Frame n is a running count of the frames written, so a run with
the switch writes ``grain.grain_stream_np`` of the stream a run without it writes, whatever the batch size; ``--crop-output pad`` pads behind
D2H, so the bars stay exact black.  One rank (the count would restart on a second; the field is a pure function of n, so handing each rank
its first n is all several ranks would take).  ``--grain 0`` builds no stage.  Not offered: measuring the grain ``--denoise`` removed and
matching it, grain correlated in time, AR-model grain as in AV1, per-plane curves, grain in linear light, several ranks,
``demfi_amd.clip``.  Without the switch no buffer, table, launch or stream is added and every byte stays the same.

``--deblock [A[:B]]`` smooths the block edges of 8x8-DCT coded input (DV, 576i / 480i captures, NTSC DVDs behind ``--ivtc``, broadcast
captures) in front of the network (``demfi_amd.deblock``): a deblurring network sharpens a block edge like any other edge and the flow sees a
grid that never moves over content that does, so the output blocks more crisply than the input and shimmers between the interpolated
instants; ``--denoise`` is purely temporal and preserves an edge that sits still.  The rule is H.264's intra-edge (bS = 4) luma filter as a
post filter on the fixed grid of 8, on every plane as a plane in its own right: a line p3 p2 p1 p0 | q0 q1 q2 q3 across an edge changes only
when |p0-q0| < a, |p1-p0| < b and |q1-q0| < b, up to three samples a side when that side is flat (|p0-q0| < (a >> 2) + 2 and |p2-p0| < b), one
otherwise; all vertical edges first, then all horizontal ones on that result.  A and B are 8-bit steps (0 <= B <= A <= 255, default 16:4, A
alone is A : (A + 3) // 4, one pair for every plane, shifted to the working depth); ``--deblock 0`` builds no stage.  The stage sits at the top
of the ingest, H2D -> promote (``--work-depth``) -> deblock -> bob / adaptive -> denoise -> frames, tiles, scene scores, dedup probe: ONE
launch per run of consecutive newly uploaded slots (csrc/deblock.hip ``demfi_payload_deblock``, byte for byte
``deblock.deblock_payload_np``) works in place on the uploaded payloads, a workgroup per tile whose borders lie half way between edges, so a
run with the switch writes the bytes of a run without it over the stream deblocked on the host.  Under ``--deinterlace`` (either mode) each
field of each plane is filtered as a plane of its own, edges every 8 field rows, so nothing is averaged across two time instants; behind
``--ivtc`` the film frames are progressive and filtered as such.  With ``--crop`` the grid belongs to the uncropped stream: the rectangle's top
and left give the phases.  ``--ivtc`` and ``--crop auto`` decide in front of the device, on the input's own samples.  The stage keeps nothing
between payloads and needs no look-ahead: every switch above and several ranks work, ``--dedup`` and ``--deinterlace-mode adaptive`` included.
Not offered: frame-DCT blocks of interlaced material, whose edges fall every 4 field rows; grids other than 8, and material scaled after
coding; strength from a quantiser, and per-plane thresholds; ``demfi_amd.clip``; numeric equality with ffmpeg's ``deblock`` / ``pp``;
ringing is the business of ``--dering``.  Without the switch no buffer, table, launch or counter is added and every byte stays the same.

``--dering [P[:S[:D]]]`` removes the other artefact of 8x8-DCT coded input, ringing and mosquito noise beside strong edges, in front of the
network (``demfi_amd.dering``): a deblurring network sharpens the ripples like any other fine detail, and because they change with the
coder's quantiser from frame to frame the flow sees motion that is not there; ``--denoise`` stops at any difference above A, which ringing
beside a moving edge always is, and ``--deblock`` touches only samples within 3 of a grid line.  The rule is AV1's constrained directional
enhancement filter (CDEF) in exact integers, on every plane as a plane in its own right: every 8x8 block of the coder's grid finds the
dominant one of 8 directions, a sample is smoothed strongly along it (4 primary taps, strength P scaled by the block's directional
variance, none in a flat block) and weakly across it (8 secondary taps, strength S), every tap through a constraint function that leaves it
alone when it differs from the centre by more than the strength allows (damping D), so real edges stay, and the result is clamped to the
extremes of what it read.  P (0 .. 15), S (0 .. 4) and D (3 .. 6) are 8-bit steps, one triple for every plane, shifted to the working depth;
the default 4:2:5 is the middle of AV1's range and has not been tuned against this network; P alone is P : min((P + 1) // 2, 4) : 5;
``--dering 0:0`` builds no stage.  The stage sits behind the deblocker, H2D -> promote (``--work-depth``) -> deblock -> dering -> bob /
adaptive -> denoise -> frames, tiles, scene scores, dedup probe: the filter reads a halo of unfiltered samples and cannot work in place, so
per run of consecutive newly uploaded slots one device copy takes the payloads into a scratch buffer and ONE launch (csrc/dering.hip
``demfi_payload_dering``, byte for byte ``dering.dering_payload_np``) writes them back deringed; a run with the switch writes the bytes of a
run without it over the stream deringed on the host.  Under ``--deinterlace`` (either mode) each field of each plane is a plane of its own;
with ``--crop`` the grid belongs to the uncropped stream.  The stage keeps nothing between payloads and needs no look-ahead: every switch
above and several ranks work.  Not offered: equality with libaom / dav1d output (the strengths are per stream and not per superblock, every
plane searches its own direction, there is no skip map); strength from a quantiser; per-plane strengths; 4x4 chroma blocks; frame-DCT
blocks of interlaced material; ``demfi_amd.clip``.  Without the switch no buffer, table, launch, copy or counter is added and every byte
stays the same.

``--deband [T[:R]]`` removes the third artefact of low-bitrate 8-bit input, banding, in front of the network (``demfi_amd.deband``): a sky, a
wall or a fade arrives as plateaus one code apart; the promotion to the working depth is a pure shift and keeps the steps (4 codes at 10
bits), the network sharpens a contour of one code like any other edge, and the egress can only bury it in grain.  The rule is a
range-limited box mean (Lee's sigma filter with a hard threshold) in exact integers, on every plane as a plane in its own right: a sample
becomes the mean, rounded to nearest, of the samples of its (2R + 1)^2 window that differ from it by less than T, the window clipped
symmetrically about the sample at the plane's borders, so every affine plane comes back exactly and a step of T or more stays an edge.  T
(0 .. 8) is in 8-bit steps, shifted to the working depth, R (1 .. 16) in samples, one pair for every plane; the default 2:16 has not been
tuned against this network; T alone is T:16; ``--deband 0`` builds no stage.  At equal input and working depth a band of one code rounds
back to itself: the switch wants ``--work-depth 10`` or more on 8-bit input (it is not refused without).  Bands narrower than about R / T
come back unchanged, plateaus of 16 to 32 samples come back as ramps with steps of at most one code; fine detail within T is averaged like
a band (``profiles/deband.md`` has the price).  The stage sits directly behind the deringing filter, H2D -> promote -> deblock -> dering ->
deband -> bob / adaptive -> denoise -> frames, tiles, scene scores, dedup probe: per run of consecutive newly uploaded slots one device
copy takes the payloads into the scratch buffer (the deringing filter's where both switches are given) and ONE launch (csrc/deband.hip
``demfi_payload_deband``, byte for byte ``deband.deband_payload_np``) writes them back; a run with the switch writes the bytes of a run
without it over the stream debanded on the host.  Under ``--deinterlace`` (either mode) each field of each plane is a plane of its own and R
counts field rows.  The stage keeps nothing between payloads and needs no look-ahead: every switch above and several ranks work.  Not
offered: debanding behind ``--denoise`` (that stage is deferred and has its own buffer); randomly placed reference samples in the manner of
``f3kdb`` / ffmpeg's ``deband``; dither or grain at this stage (``--grain`` is the place); per-plane pairs; a radius above 16; bands narrower
than about R / T; ``demfi_amd.clip``; numeric equality with any ffmpeg filter.  Without the switch no buffer, table, launch, copy or counter
is added and every byte stays the same.

``--lut FILE.cube`` applies a user's 3D colour LUT to every payload written (``demfi_amd.lut3d``): the edge's colour side stops at two
transfer curves and two matrices, and a cube covers HDR10 or HLG to SDR, BT.2020 to BT.709, camera log to display, a legaliser or a look
without the project defining any of them.  With the switch the egress runs on RGB payloads (uint16 [3, h, w], the format of
``--linear-light``) whether or not the run is in linear light: gather-to-RGB -> mix -> scale -> lut -> encode -> grain -> weave -> requant
-> D2H.  The gather writes through ``colour.forward_table`` in linear light and through ``lut3d.code_table`` otherwise, the LUT reads through
the inverse of that same table and writes 16-bit encoded values, the encode reads those through ``inverse_table(code_table)``;
``demfi_bgr_to_linear_gather`` and ``demfi_linear_to_yuv`` are reused unchanged.  ONE launch per batch (csrc/lut3d.hip ``demfi_rgb_lut3d``, byte
for byte ``lut3d.lut_payload_np``): tetrahedral interpolation in exact integers, the cube quantised to 16 bits (values outside [0, 1]
clipped).  An identity cube of any size returns every code, so a run without ``--shutter`` and ``--scale`` writes the bytes of the run without
the switch.  ``--out-matrix`` and ``--out-range`` bind the encode as before; ``--crop-output pad`` pads behind D2H, so the bars stay exact
black whatever the cube does to black.  Stateless per payload: any number of ranks.  Refused before anything is allocated: a file that does
not parse (with its line) and a working depth above 12 bits (the gather keeps its table of at most 4096 entries in LDS, as for
``--linear-light``; see ``--work-depth``).  Not offered: a LUT in front of the network (log or HDR sources), 1D and shaper LUTs, domains
other than 0 .. 1, trilinear interpolation, other file formats, a transfer or primaries tag in the header (Y4M has none), working depths
14 and 16, ``demfi_amd.clip``, numeric equality with ffmpeg's ``lut3d`` or OCIO.  Without the switch no buffer, table, launch or counter is
added and every byte stays the same.

``--nlmeans [S[:P[:R]]]`` denoises every plane within the frame, in front of the network (``demfi_amd.nlmeans``): ``--denoise`` is purely
temporal and stops at the first difference above A, so on a moving object, a pan or a zoom every sample keeps its grain, and those are the
samples the flow estimator works on.  The rule is non-local means in exact integers, on every plane as a plane in its own right: a sample
becomes the weighted mean, rounded to nearest, of the samples of its (2R + 1)^2 search window that lie inside the plane, each weighed by a
table of 1024 entries (built on the host, 256 exp(-D / (np_ 4^b S^2))) of the summed squared difference D of the (2P + 1)^2 patches around
the two, the patches replicating the plane's edge.  A patch that differs by more than the table's reach weighs nothing, so a hard edge is
not seen across; no clip is needed.  S (0 .. 16) is in 8-bit steps, P (1 .. 3) and R (1 .. 7) in samples, one triple for every plane; the
default 3:2:5 has not been tuned against this network; S alone is S:2:5; ``--nlmeans 0`` builds no stage.  The filter's reach, not bugs: a
window cut off by a border or an edge is lopsided, so a ramp next to one is biased by a few codes, and a high S costs texture
(``profiles/nlmeans.md`` has the figures).  The stage sits directly behind the deringing filter and in front of the debander (noise hides
bands and denoising uncovers them), H2D -> promote -> deblock -> dering -> nlmeans -> deband -> bob / adaptive -> denoise -> frames, tiles,
scene scores, dedup probe: per run of consecutive newly uploaded slots one device copy takes the payloads into the scratch buffer (the one
the deringing filter and the debander use where they are given) and ONE launch (csrc/nlmeans.hip ``demfi_payload_nlmeans``, byte for byte
``nlmeans.nlmeans_payload_np``) writes them back; a run with the switch writes the bytes of a run without it over the stream filtered on
the host.  Under ``--deinterlace`` (either mode) each field of each plane is a plane of its own.  The stage keeps nothing between payloads
and needs no look-ahead: every switch above and several ranks work.  Not offered: separate luma / chroma strengths; a noise estimate that
sets S; temporal or motion-compensated search (that remains ``--denoise``'s side); P above 3 or R above 7; subtraction of the noise variance
from D; numeric equality with ffmpeg's ``nlmeans``; ``demfi_amd.clip``; decisions of ``--ivtc`` / ``--crop auto`` on filtered samples (they
decide in front, on the input's own).  Without the switch no buffer, table, launch, copy or counter is added and every byte stays the same.
"""
import os
import sys
from fractions import Fraction

import torch

from . import _lib as L
from . import bitdepth as BD
from . import cadence as K
from . import colour as CL
from . import deband as BA
from . import deblock as DB
from . import deint as I
from . import denoise as DN
from . import dering as DR
from . import dist as D
from . import grain as GR
from . import interlace as IL
from . import letterbox as LB
from . import lut3d as LU
from . import nlmeans as NL
from . import retime as R
from . import scale as SC
from . import scene as S
from . import shutter as SH
from . import telecine as TC
from . import tiling as T
from . import y4m
from .clip import ClipRunner
from .pipeline import KeptFrames, deint_conflict


class YuvEdge:
    """Y4M edge of ``WindowRunner.run_clip_u8``: conversion parameters of the stream (library codes), ``with_s1(k)``: does
    window k (index in the runner's window sequence) close the stream, i.e. is its S1 written?  ``scene_cut``: None, or the
    threshold T of scene-cut detection (``demfi_amd.scene``).  ``full_length``: the full-length timeline (``retime``).
    ``depth``: bits per sample, 8, or 10 / 12 / 14 / 16 for payloads of 16-bit samples.  ``layout``: the payloads' chroma
    layout, one of ``y4m.LAYOUTS`` (``siting`` only matters to '420').  ``dedup``: None, or (hi, lo, frac, max_hold) of
    repeated-frame detection (``demfi_amd.cadence``).  ``fields``: None, or the field order 't' / 'b' of an interlaced input whose
    fields are the stream's frames (``demfi_amd.deint``), rebuilt by ``deint_mode`` 'bob' or 'adaptive'.  ``shutter``: None, or (S, D) of a
    synthesized shutter (``demfi_amd.shutter``): the runner then has the fine ratio r D and the payloads handed out are the mixed ones.
    ``interlace``: None, or the field order ('tff' / 'bff' / 't' / 'b') of interlaced output (``demfi_amd.interlace``) with the low-pass mode
    ``interlace_lowpass`` (None: 'linear'; an error without ``interlace``): the payloads handed out are the woven pairs.  ``scale``: None, or
    (w, h) or (w, h, filter) of resized output (``demfi_amd.scale``; ``scale_filter`` names the filter of a pair, None: 'lanczos3'): the
    payloads handed out have that size.  ``depths``: None, or (input depth, working depth, output depth, dither mode or None) of
    ``bitdepth.resolve``: the payloads handed in have the input's depth, ``depth`` is then the WORKING depth, and the payloads handed out
    have the output's.  ``shutter_window``: None ('box') or 'triangle', the weights of the shutter's mix (``shutter.window_weights``); an
    error without ``shutter``.  ``denoise``: None, or (A, B, R) of the temporal denoiser in front of the network (``demfi_amd.denoise``).
    ``linear_light``: None, or the transfer ('bt709' / 'srgb'; True: 'bt709') through which the mix and the scaler work in linear light
    (``demfi_amd.colour``); ``out_matrix`` ('bt601' / 'bt709') and ``out_range`` ('limited' / 'full'): None, or the matrix and range of the
    payloads handed out, where ``matrix`` and ``full_range`` are those of the payloads handed in.  ``colour`` = (transfer, out matrix, out
    full range), or None without the three.  ``grain``: None, or (S16, r, C16, curve, seed) of the film grain added to every progressive payload
    in front of the weave (``demfi_amd.grain``); S16 = 0 is None.  ``deblock``: None, or (A, B) of the deblocking filter at the top of the ingest
    (``demfi_amd.deblock``); A = 0 is None.  ``crop_rect``: None, or the rectangle (top, bottom, left, right) the payloads handed in were cropped
    to out of their stream, which shifts the block grid of both.  ``dering``: None, or (P, S, D) of the deringing filter behind the deblocker
    (``demfi_amd.dering``); P = S = 0 is None.  ``deband``: None, or (T, R) of the debanding filter behind that (``demfi_amd.deband``); T = 0 is
    None.  ``lut``: None, or the ``lut3d.Cube`` (or the path of a ``.cube`` file) of the 3D colour LUT applied between the scaler and the encode
    (``demfi_amd.lut3d``).  ``nlmeans``: None, or (S, P, R) of the spatial denoiser between the deringing filter and the debander
    (``demfi_amd.nlmeans``); S = 0 is None."""

    def __init__(self, matrix, full_range, siting, with_s1, scene_cut=None, full_length=False, depth=8, layout='420', dedup=None,
                 fields=None, deint_mode='bob', shutter=None, interlace=None, interlace_lowpass=None, scale=None, scale_filter=None,
                 depths=None, shutter_window=None, denoise=None, linear_light=None, out_matrix=None, out_range=None, grain=None,
                 deblock=None, crop_rect=None, dering=None, deband=None, lut=None, nlmeans=None):
        self.nlmeans = check_nlmeans(nlmeans)
        self.dedup, self.shutter = dedup, shutter
        self.lut = check_lut(lut)
        self.deblock = check_deblock(deblock)
        self.dering = check_dering(dering)
        self.deband = check_deband(deband)
        self.crop_rect = None if crop_rect is None else tuple(int(v) for v in crop_rect)
        self.grain = None if grain is None or not GR.check_params(grain)[0] else GR.check_params(grain)
        self.colour = check_colour(linear_light, out_matrix, out_range)
        self.denoise = None if denoise is None else DN.check_params(*denoise)
        self.shutter_window = check_shutter_window(shutter, shutter_window)
        self.depths = None if BD.is_noop(depths) else tuple(depths)
        if self.depths is not None and self.depths[1] != depth:
            raise ValueError('YuvEdge: depths=%r with depth=%r: depth is the working depth' % (self.depths, depth))
        if scale is not None and len(scale) == 3 and scale_filter is None:
            scale, scale_filter = tuple(scale[:2]), scale[2]
        self.scale = check_scale(scale, scale_filter)
        self.interlace = check_interlace(interlace, interlace_lowpass)
        self.fields, self.deint_mode = fields, deint_mode
        self.depth = y4m.check_depth(depth)
        self.layout = y4m.check_layout(layout)
        self.matrix = {'bt601': L.BT601, 'bt709': L.BT709}[matrix]
        self.full_range = bool(full_range)
        self.siting = {'420jpeg': L.SITING_420JPEG, '420mpeg2': L.SITING_420MPEG2}[siting]
        self.with_s1 = with_s1
        self.scene_cut = scene_cut
        self.full_length = full_length


ONE_RANK = {        # the switches that run on one rank only, and why
    'dedup': 'which frames are kept depends on the whole prefix of the input, so a rank cannot place its block of windows from k and r alone',
    'ivtc': 'which frames are dropped depends on the whole prefix of the input, so a rank cannot place its block of windows from k and r alone',
    'shutter': 'the sub-frames of a written frame straddle the ranks\' blocks of windows',
    'interlace': 'the two frames of a written payload can straddle the ranks\' blocks of windows',
}


# and of the egress stages that came after: kept the same way, in a table of their own
ONE_RANK_EGRESS = {
    'grain': 'frame n of the grain is a running count of the frames a rank writes, so a second rank would restart it (the field is a pure '
             'function of n: handing each rank its first n is all it would take)',
}


def check_one_rank(world, **switches):
    """The switches of ``ONE_RANK`` and ``ONE_RANK_EGRESS`` that are set (neither None nor False) are refused with more than one rank."""
    for name, why in (*ONE_RANK.items(), *ONE_RANK_EGRESS.items()):
        if world > 1 and switches.get(name) not in (None, False):
            raise ValueError('VideoRunner: %s with %d ranks: %s; run --%s on one rank' % (name, world, why, name))


def check_ivtc(ivtc, deinterlace):
    """``--ivtc`` does not go with ``--deinterlace``."""
    if ivtc and deinterlace:
        raise ValueError('--ivtc does not go with --deinterlace: inverse telecine puts the fields of a film frame back together, the '
                         'deinterlacer makes a frame of every field; choose one (film carried by 3:2 pulldown: --ivtc)')


def check_crop(crop, limit=LB.DEFAULT_LIMIT, noise=LB.DEFAULT_NOISE, probe=LB.DEFAULT_PROBE, output='pad'):
    """The crop switches checked: (crop, (limit, noise, probe, output)).  The four secondary ones say how ``crop`` works, so any of
    them without it is an error."""
    crop, params = LB.check_crop(crop), LB.check_params(limit, noise, probe, output)
    if crop is None and params != (LB.DEFAULT_LIMIT, LB.DEFAULT_NOISE, LB.DEFAULT_PROBE, 'pad'):
        raise ValueError('--crop-limit, --crop-noise, --crop-probe and --crop-output (crop_limit, crop_noise, crop_probe, crop_output) '
                         'say how --crop works: give --crop auto or --crop T:B:L:R with them')
    return crop, params


def check_shutter(shutter, samples=None, dedup=None, world=1):
    """The shutter switches checked: None, or (S, D) of ``shutter.check_params``.  ``samples`` (None: the default) says how ``shutter``
    works, so it is an error without it; a shutter does not go with ``--dedup`` or with more than one rank."""
    if shutter is None:
        if samples is not None:
            raise ValueError('--shutter-samples (shutter_samples) says how --shutter works: give --shutter ANGLE with it')
        return None
    sd = SH.check_params(shutter, SH.DEFAULT_SAMPLES if samples is None else samples)
    if dedup not in (None, False):
        raise ValueError('--shutter does not go with --dedup: the sub-frames of a written frame are laid over the regular fine timeline, which '
                         'repeated frames left out of the input bend; run one of the two')
    check_one_rank(world, shutter=sd)
    return sd


def check_shutter_window(shutter, window=None):
    """The shutter's window checked: 'box' or 'triangle' (``shutter.WINDOWS``; None: 'box'), or None without a shutter.  ``window`` says how
    ``shutter`` works, so it is an error without it."""
    if shutter is None:
        if window is not None:
            raise ValueError('--shutter-window (shutter_window) says how --shutter works: give --shutter ANGLE with it')
        return None
    return SH.check_window(window)


def check_interlace(interlace, lowpass=None, world=1):
    """The interlace switches checked: None, or (field order 't' / 'b', low-pass mode).  ``lowpass`` (None: 'linear') says how ``interlace``
    works, so it is an error without it; interlaced output runs on one rank."""
    if interlace is None:
        if lowpass is not None:
            raise ValueError('--interlace-lowpass (interlace_lowpass) says how --interlace works: give --interlace tff or bff with it')
        return None
    il = (IL.parse_order(interlace), IL.check_lowpass(lowpass))
    check_one_rank(world, interlace=il)
    return il


def check_scale(scale, scale_filter=None, crop=None, crop_output='pad'):
    """The scale switches checked: None, or (w, h, filter).  ``scale`` is (w, h) or a 'WxH' string, width first; ``scale_filter`` (None:
    'lanczos3') says how ``scale`` works, so it is an error without it.  With ``crop`` the picture rectangle is what gets scaled, so
    the output must be the cropped one."""
    if scale is None:
        if scale_filter is not None:
            raise ValueError('--scale-filter (scale_filter) says how --scale works: give --scale WxH with it')
        return None
    w, h = SC.parse_size(scale) if isinstance(scale, str) else SC.check_size(scale)
    if crop is not None and crop_output != 'cropped':
        raise ValueError('--scale with --crop needs --crop-output cropped (crop_output=\'cropped\'): the picture rectangle is what is scaled, '
                         'and with pad the bars would have to go back around a picture of another size')
    return w, h, SC.check_filter(scale_filter)


def check_colour(linear_light=None, out_matrix=None, out_range=None, auto=False):
    """The colour switches checked: None without them, or (transfer or None, out matrix or None, out full range or None).  'auto' as the
    output matrix is the ``VideoRunner``'s to resolve (it knows the height written): only with ``auto``."""
    transfer, matrix, rng = CL.check_switches(linear_light, out_matrix, out_range)
    if matrix == 'auto' and not auto:
        raise ValueError("out_matrix='auto' is resolved by VideoRunner from the height written; give 'bt601' or 'bt709' here")
    if transfer is None and matrix is None and rng is None:
        return None
    return transfer, matrix, None if rng is None else rng == 'full'


def check_depths(work_depth=None, out_depth=None, dither=None):
    """The bit-depth switches checked as far as they can be before a header is known (``bitdepth.check_switches``): depths of
    ``y4m.DEPTHS``, D <= W, and ``dither`` ('bayer' / 'none'; None: 'bayer') says how a requantisation rounds, so it is an error without
    either depth.  What depends on the input's depth (W below it, a ``dither`` where the output ends at the working depth) is refused by
    ``bitdepth.resolve`` once the header is known, before anything is allocated.  Returns (work_depth, out_depth, dither)."""
    return BD.check_switches(work_depth, out_depth, dither)


def check_denoise(denoise, radius=None, dedup=None, deinterlace_mode='bob'):
    """The denoise switches checked: None, or (A, B, R) of ``denoise.check_params``.  ``denoise``: None / False (off), True (the defaults
    5:10), A (A:2A), (A, B) or an "A[:B]" string; ``radius`` (None: 2) says how ``denoise`` works, so it is an error without it.  The
    denoiser does not go with ``--dedup`` or with ``--deinterlace-mode adaptive``."""
    if denoise is None or denoise is False:
        if radius is not None:
            raise ValueError('--denoise-radius (denoise_radius) says how --denoise works: give --denoise [A[:B]] with it')
        return None
    if denoise is True:
        denoise = DN.DEFAULTS
    elif isinstance(denoise, str):
        denoise = DN.parse_denoise(denoise)
    elif isinstance(denoise, int):
        denoise = (denoise, None)
    if not isinstance(denoise, (tuple, list)) or len(denoise) != 2:
        raise ValueError('denoise must be None, True, A, (A, B) or "A[:B]", got %r' % (denoise,))
    dn = DN.check_params(denoise[0], denoise[1], radius)
    if dedup not in (None, False):
        raise ValueError('--denoise does not go with --dedup: repeated frames are staged and discarded one frame at a time, the denoiser '
                         'needs the frames after the one it cleans; run one of the two')
    if deinterlace_mode != 'bob':
        raise ValueError('--denoise does not go with --deinterlace-mode %s: both wait for frames ahead and the first rebuilds its payloads in '
                         'place; use --deinterlace-mode bob with --denoise' % deinterlace_mode)
    return dn


def check_deblock(deblock):
    """The deblock switch checked: None (off, or A = 0: no stage), or (A, B) of ``deblock.check_params``.  ``deblock``: None / False (off), True
    (the defaults 16:4), A (A : (A + 3) // 4), (A, B) or an "A[:B]" string.  Goes with every other switch and any number of ranks."""
    if deblock is None or deblock is False:
        return None
    if deblock is True:
        deblock = DB.DEFAULTS
    elif isinstance(deblock, str):
        deblock = DB.parse_deblock(deblock)
    elif isinstance(deblock, int):
        deblock = (deblock, None)
    if not isinstance(deblock, (tuple, list)) or len(deblock) != 2:
        raise ValueError('deblock must be None, True, A, (A, B) or "A[:B]", got %r' % (deblock,))
    ab = DB.check_params(deblock[0], deblock[1])
    return ab if ab[0] else None


def check_dering(dering):
    """The dering switch checked: None (off, or P = S = 0: no stage), or (P, S, D) of ``dering.check_params``.  ``dering``: None / False (off),
    True (the defaults 4:2:5), P (P : min((P + 1) // 2, 4) : 5), (P, S), (P, S, D) or a "P[:S[:D]]" string.  Goes with every other switch and
    any number of ranks."""
    if dering is None or dering is False:
        return None
    if dering is True:
        dering = DR.DEFAULTS
    elif isinstance(dering, str):
        dering = DR.parse_dering(dering)
    elif isinstance(dering, int):
        dering = (dering,)
    if not isinstance(dering, (tuple, list)) or not 1 <= len(dering) <= 3:
        raise ValueError('dering must be None, True, P, (P, S), (P, S, D) or "P[:S[:D]]", got %r' % (dering,))
    psd = DR.check_params(*dering)
    return psd if psd[0] or psd[1] else None


def check_nlmeans(nlmeans):
    """The nlmeans switch checked: None (off, or S = 0: no stage), or (S, P, R) of ``nlmeans.check_params``.  ``nlmeans``: None / False
    (off), True (the defaults 3:2:5, not tuned against this network), S (S:2:5), (S, P, R) or a "S[:P[:R]]" string.  Goes with every other
    switch and any number of ranks."""
    if nlmeans is None or nlmeans is False:
        return None
    if nlmeans is True:
        nlmeans = NL.DEFAULTS
    elif isinstance(nlmeans, str):
        nlmeans = NL.parse_nlmeans(nlmeans)
    elif isinstance(nlmeans, int):
        nlmeans = (nlmeans,)
    if not isinstance(nlmeans, (tuple, list)) or not 1 <= len(nlmeans) <= 3:
        raise ValueError('nlmeans must be None, True, S, (S, P, R) or "S[:P[:R]]", got %r' % (nlmeans,))
    spr = NL.check_params(*nlmeans)
    return spr if spr[0] else None


def check_deband(deband):
    """The deband switch checked: None (off, or T = 0: no stage), or (T, R) of ``deband.check_params``.  ``deband``: None / False (off),
    True (the defaults 2:16), T (T:16), (T, R) or a "T[:R]" string.  Goes with every other switch and any number of ranks."""
    if deband is None or deband is False:
        return None
    if deband is True:
        deband = BA.DEFAULTS
    elif isinstance(deband, str):
        deband = BA.parse_deband(deband)
    elif isinstance(deband, int):
        deband = (deband,)
    if not isinstance(deband, (tuple, list)) or not 1 <= len(deband) <= 2:
        raise ValueError('deband must be None, True, T, (T, R) or "T[:R]", got %r' % (deband,))
    tr = BA.check_params(*deband)
    return tr if tr[0] else None


def check_lut(lut=None, work_depth=None):
    """The LUT switch checked: None, or the ``lut3d.Cube`` of ``lut`` -- a ``Cube`` as it is, else the path of a ``.cube`` file, read and parsed
    here (ValueError with the file's name and the line for one that does not parse).  ``work_depth``: the working depth where it is known;
    above 12 bits it is refused in ``lut3d.check_depth``'s words, which point to ``--work-depth``."""
    if lut is None:
        return None
    if work_depth is not None:
        LU.check_depth(work_depth)
    return lut if isinstance(lut, LU.Cube) else LU.load_cube(os.fspath(lut))


def check_grain(grain=None, size=None, chroma=None, curve=None, seed=None, world=1):
    """The grain switches checked: None (no ``grain``, or S = 0: no stage) or (S16, r, C16, curve, seed) of ``grain.check_grain``.  ``grain``:
    S as a number or a decimal string, 0 .. 8; ``size`` 0, 1 or 2 (None: 1); ``chroma`` C in 0 .. 1 (None: 0.5); ``curve`` 'film' / 'flat' (None:
    'film'); ``seed`` a uint32 (None: 0).  The four say how ``grain`` works, so any of them without it is an error; grain runs on one rank."""
    params = GR.check_grain(grain, size, chroma, curve, seed)
    check_one_rank(world, grain=params)
    return params


# what a run adds to each of these counters of its ``WindowRunner`` is kept in the ``VideoRunner`` attribute named here (None: it goes into
# ``last_instants`` = (run, padded), and a shutter's fine frames into ``last_st_frames``: ``VideoRunner._counted``)
COUNTERS = {'instants_run': None, 'instants_padded': None, 'shutter_mixed': None, 'cut_windows': 'last_cut_windows',
            'shutter_carried': 'last_shutter_carried', 'interlace_carried': 'last_interlace_carried', 'scale_payloads': 'last_scale_payloads',
            'depth_promoted': 'last_depth_promoted', 'depth_requantised': 'last_depth_requantised'}
# and of the egress stages that came after: linear light (``y4m_edge.Encoder``), film grain (``y4m_edge.Grain``), the 3D LUT (``y4m_edge.Lut``)
EGRESS_COUNTERS = {'colour_encoded': 'last_colour_encoded', 'grain_payloads': 'last_grain_payloads', 'lut_payloads': 'last_lut_payloads'}
# the counters of the ingest stages that came after those: kept the same way, in a table of their own
INGEST_COUNTERS = {'denoised': 'last_denoised', 'deblocked': 'last_deblocked', 'deringed': 'last_deringed', 'debanded': 'last_debanded',
                   'nlm_filtered': 'last_nlm_filtered'}


AUTO_NEEDS_A_FILE = ('--crop auto needs a regular input file: the bars of a stream are known only at its end; give the four bar '
                     'widths instead, --crop T:B:L:R (crop=(T, B, L, R)), for instance from ffmpeg -vf cropdetect')


def check_deinterlace_mode(deinterlace, mode, dedup):
    """``pipeline.deint_conflict`` in the words of the switches: 'adaptive' only with ``--deinterlace`` and not with ``--dedup``."""
    why = deint_conflict(mode, deinterlace, dedup not in (None, False))
    if why == 'mode':
        raise ValueError('deinterlace_mode must be one of %s, got %r' % (', '.join(I.MODES), mode))
    if why == 'fields':
        raise ValueError('--deinterlace-mode %s needs --deinterlace (deinterlace=True): the mode says how fields are rebuilt' % mode)
    if why == 'dedup':
        raise ValueError('--deinterlace-mode %s does not go with --dedup: repeated frames are staged and discarded one field at a time, '
                         'the %s mode needs two fields of lookahead; use --deinterlace-mode bob with --dedup' % (mode, mode))


class VideoRunner:
    """x M interpolation (``mfi``, default 8) or retiming to the output frame rate ``fps`` (a Fraction >= the input's rate; with ``down``
    at least 1/64 of it) of Y4M input on this rank's GPU; give one of the two.  ``matrix``: 'auto' (BT.709 when H >= 720, else BT.601), 'bt601'
    or 'bt709'; the output uses the input's matrix and range, so an ffmpeg round trip keeps the colours.  ``scene_cut``: None
    (default) or the threshold T in (0, 100] of scene-cut detection: no window interpolates across a cut (``demfi_amd.scene``);
    the output's timing is unchanged.  ``full_length``: the output covers the input's whole timeline (``retime``): output
    frame 0 is input frame 0, n frames give ceil(n r) (n M for x M), the clip's ends clamp the tuples like cuts and the last
    frame is held to the end.  After a run, ``last_instants`` = (time instants run, padded per-t
    slots), ``last_st_frames`` = St frames written, ``last_cuts`` = the frames j that start a scene and ``last_cut_windows`` =
    the windows run as cut windows, of this rank.  ``tile``: None, 'auto' or (th, tw): frames run as overlapping tiles
    (``demfi_amd.tiling``, ``tile_margin`` pixels thrown away next to every cut); ``last_plan`` is the plan of the last input, None
    when it ran untiled, and ``last_instants`` then counts per tile.  ``high_depth``: also take 10- to 16-bit 4:2:0 input
    (C420p10 / C420p12 / C420p14 / C420p16) and give the output at the input's depth (``last_depth``); off by default, and an
    8-bit stream gives the same bytes either way.  Together with ``tile`` only when ``tile_high_depth`` is set (off by default: a
    stream above 8 bits is then refused before anything is allocated); every tile is then read out of and written into the full
    16-bit frames in place, and the switch changes nothing for an 8-bit stream or an untiled run.  ``layouts``: also take
    4:2:2, 4:4:4 and mono input (C422, C444, Cmono; with ``high_depth`` their deep forms C422pNN / C444pNN / CmonoNN) and give the
    output in the input's layout (``last_layout``); off by default, and a 4:2:0 stream gives the same bytes either way.  Every
    layout runs with ``tile``, since tiles cut BGR frames (the deep ones with ``tile_high_depth``).  ``dedup``: None (default),
    True or (hi, lo, frac): input frames that repeat the last kept frame (``demfi_amd.cadence``: no 8x8 luma block differs by more than hi, at most frac of them by more
    than lo; True takes the defaults of ffmpeg's mpdecimate) are left out and the windows interpolate over the gap, at most
    ``dedup_max_hold`` repeats in a row; the output's length and timing are unchanged.  ``last_dups`` lists the input frames
    dropped.  One rank only: which frames are kept depends on the whole prefix of the input.  ``deinterlace``: also take
    interlaced input of a fixed field order (``It`` / ``Ib``) and bob it (``demfi_amd.deint``): field f = 2p + s of payload p is
    progressive frame f, so the input counts as 2n frames at twice its rate -- ``mfi`` multiplies and ``fps`` is checked against
    that field rate, and windows, ranks and output counts follow it; the output is progressive.  ``last_fields`` is None, 'tff'
    or 'bff'.  Off by default (an interlaced stream is refused before anything is allocated); a progressive stream gives the same
    bytes either way.  ``deinterlace_mode``: 'bob' (default) or 'adaptive', the motion-adaptive rule of ``demfi_amd.deint`` over fields
    f-2 .. f+2; only with ``deinterlace``, and not with ``dedup`` (both are refused here, before anything is allocated).  ``ivtc``: inverse
    telecine (``demfi_amd.telecine``): the input, whatever its I tag, is field-matched and decimated to n - floor(n/5) progressive
    frames at 4/5 of its rate before anything else sees it; ``mfi`` multiplies and ``fps`` is checked against that film rate.
    ``ivtc_cthresh`` (0..255, default 9) is the comb threshold, ``ivtc_combpel`` (0..256, default 80) the combed samples of a 16x16
    block above which a matched frame counts as combed, ``ivtc_combed`` what happens to such a frame: 'bob' (default) or 'keep'.
    One rank only, and not with ``deinterlace`` (refused here).  After a run ``last_matches`` = {'c': , 'p': , 'n': } counts of the
    payloads' matches, ``last_dropped`` = the input payloads dropped, ``last_combed`` = the film frames left combed.  Off by
    default: nothing changes anywhere without it.  ``crop``: None (default), 'auto' or the bar widths (T, B, L, R) in luma samples
    (``demfi_amd.letterbox``): the payloads are cropped to the picture rectangle in front of everything that runs on the GPU and the
    outputs are padded back with black (``crop_output`` 'pad', default) or written at the cropped size ('cropped').  'auto' finds the
    rectangle in a pre-pass over the luma planes of ``crop_probe`` ('all', or N payloads spread over the input) with the limit
    ``crop_limit`` (8-bit steps, default 24) and the allowance ``crop_noise`` (a Fraction of a line, default 1/256); it needs a regular
    file (``run_file``) and is refused on ``run_stream`` before anything is allocated; the four numbers work everywhere and launch
    nothing.  An explicit rectangle that is misaligned (top and left on the chroma grid, rows in units of 4 for interlaced 4:2:0) or
    keeps fewer than 64 rows or columns is a ValueError once the header is known, before a library is loaded.  After a run
    ``last_crop`` = (top, bottom, left, right) or None when nothing was cropped, ``last_crop_probed`` = payloads probed,
    ``last_crop_note`` = None or why an 'auto' rectangle was not used.  Not offered: bars that change within a stream (the union is
    taken), restoring the input's own bar samples (output bars are exact black); scene cuts and repeated frames are decided over the
    cropped payloads, so they can differ from those of an uncropped run.  The four secondary arguments without ``crop`` are an
    error; without ``crop`` nothing changes anywhere: no buffer, stream or launch is added.  ``shutter``: None (default) or the shutter
    angle in degrees (an int, a Fraction or an "N/D" string, 0 < angle <= 360) of synthesized motion blur (``demfi_amd.shutter``) with
    ``shutter_samples`` = S sub-frames (1 .. 32; None, the default, is 4; given without ``shutter`` it is an error): every written frame is the
    rounded average of the fine frames c D .. c D + S - 1, D = 360 S / angle (an integer, or a ValueError here), of the stream at the
    ratio r D, which is refused above ``retime.MAX_RATIO`` once the header is known, before anything is allocated.  Not with ``dedup``
    (refused here) and on one rank (``run_file`` refuses more).  After a run ``last_shutter`` = (S, D) or None, ``last_instants`` counts
    the instants that ran (those the written frames need), ``last_st_frames`` the fine frames that went into the mixes and
    ``last_shutter_carried`` the samples that were carried from one batch to the next on the device.  ``interlace``: None (default), or
    'tff' / 'bff' ('t' / 'b'): interlaced output (``demfi_amd.interlace``).  Frames 2q and 2q + 1 of the progressive stream a run without the
    switch writes (with ``shutter``: its mixed frames) become the first and the second field of written payload q, an odd last frame is woven
    with itself, and the header says ``It`` / ``Ib`` at half the rate: ``mfi`` and ``fps`` name the field rate.  ``interlace_lowpass``: None (the
    default, 'linear'), 'off', 'linear' or 'complex', the vertical filter against interline twitter, within each field's own frame; given
    without ``interlace`` it is an error.  ONE launch per batch weaves (csrc/interlace.hip ``demfi_payload_weave``), the one open frame is
    carried on the device and only woven payloads cross D2H.  A ``crop`` rectangle must then keep field parity: rows in units of 2 (4 for
    4:2:0).  One rank (``run_file`` refuses more).  After a run ``last_interlace`` = 't', 'b' or None and ``last_interlace_carried`` = the
    frames carried from one batch to the next.  Without it no buffer, launch or stream is added and every byte stays the same.  ``scale``:
    None (default), (w, h) or a 'WxH' string, width first: resized output (``demfi_amd.scale``).  Every progressive payload the run would
    write is resampled to w x h on the GPU, behind the gather and the shutter's mix and in front of the weave, by ONE launch per batch
    (csrc/scale.hip ``demfi_payload_scale``); the header gets the size and the pixel aspect that keeps the display aspect.
    ``scale_filter``: None (the default, 'lanczos3'), 'lanczos3', 'bicubic' or 'bilinear'; given without ``scale`` it is an error.  With
    ``crop`` only under ``crop_output='cropped'`` (refused here); with ``interlace`` h must be a multiple of 2 (4 for 4:2:0), and a shrink
    takes at most 32 taps an axis (both refused once the header is known, before anything is allocated).  A size equal to the run's own
    builds no stage.  Any number of ranks.  After a run ``last_scale`` = (w, h, filter), or None when nothing was resized, and
    ``last_scale_payloads`` = the payloads resampled.  Without it no buffer, launch or stream is added and every byte stays the same.
    ``work_depth``, ``out_depth``: None (default) or a depth of ``y4m.DEPTHS`` (``demfi_amd.bitdepth``): the depth every stage computes at
    (payloads are promoted on the GPU right behind their upload; default max(input depth, ``out_depth``)) and the depth written (requantised
    on the GPU as the last device stage; default the INPUT's depth, so ``work_depth=12`` alone is 8 -> 12 -> 8).  ``dither``: None (the
    default, 'bayer'), 'bayer' or 'none', how a requantisation rounds; given without either depth it is an error here, and where the output
    ends at the working depth once the header is known, like a ``work_depth`` below the input's depth; ``out_depth`` above ``work_depth`` is
    refused here.  An input above 8 bits still needs ``high_depth``; with ``tile`` a working depth above 8 needs ``tile_high_depth``.  Any
    number of ranks.  After a run ``last_depth`` = the depth written, ``last_depths`` = (input, working, output depth, dither mode or None),
    or None when nothing changed, ``last_depth_promoted`` / ``last_depth_requantised`` = the payloads that went through the two stages.
    Depths that resolve to the input's add no buffer, launch or stream and every byte stays the same.  ``down``: False (default) or True:
    ``fps`` may lie below the input's rate (behind ``deinterlace`` below the field rate, behind ``ivtc`` below the film rate), r = F_out /
    F_in in 1/64 .. 1 (``retime.ratio(..., down=True)``).  The timeline is ``retime``'s; a window that owns no output runs nothing and
    ``last_windows_skipped`` counts those of the last run.  Not with ``dedup`` below the input rate (refused once the header is known);
    with ``fps`` at or above the input's rate nothing changes.  ``shutter_window``: None (the default, 'box'), 'box' or 'triangle', the
    weights of the shutter's samples (``shutter.window_weights``); given without ``shutter`` it is an error.  After a run
    ``last_shutter_window`` = 'box', 'triangle' or None without a shutter.  ``denoise``: None (default), True (the thresholds 5:10), A
    (A:2A), (A, B) or an "A[:B]" string, at the 8-bit scale with 0 <= A <= B <= 255: the temporal denoiser in front of the network
    (``demfi_amd.denoise``) with ``denoise_radius`` = R frames on each side (1 .. 3; None, the default, is 2; given without ``denoise`` it is
    an error).  Every frame is denoised on the GPU behind the promotion and the bob (csrc/denoise.hip ``demfi_payload_denoise``, ONE launch
    per batch) and everything behind that, scene cuts included, runs on the denoised stream.  Not with ``dedup`` or
    ``deinterlace_mode='adaptive'`` (refused here).  Any number of ranks.  After a run ``last_denoised`` = the frames denoised.  Without it
    no buffer, table, launch or slot is added and every byte stays the same.  ``linear_light``: None (default), True / 'bt709' or
    'srgb': the shutter's mix and the scaler work in linear light through that transfer (``demfi_amd.colour``); ``out_matrix``: None (the
    input's), 'auto' (by the height written), 'bt601' or 'bt709'; ``out_range``: None (the input's), 'limited' or 'full'.  Linear light at a
    working depth above 12 bits is refused once the header is known.  After a run ``last_colour`` = (transfer or None, matrix, full range)
    the run wrote with, or None without the three, and ``last_colour_encoded`` = the payloads the encode stage took back.  ``grain``: None
    (default) or S, the standard deviation in 8-bit code values (a number or a decimal string, 0 .. 8, in sixteenths) of synthetic film
    grain (``demfi_amd.grain``) added on the GPU to every progressive payload behind the mix, the scaler and the encode and in front of the
    weave and the requantisation (csrc/grain.hip ``demfi_payload_grain``, ONE launch per batch); ``grain_size`` 0, 1 or 2 (None: 1),
    ``grain_chroma`` C in 0 .. 1 (None: 0.5), ``grain_curve`` 'film' / 'flat' (None: 'film'), ``grain_seed`` a uint32 (None: 0); any of the four
    without ``grain`` is an error.  One rank (``run_file`` refuses more).  ``grain=0`` builds no stage.  After a run ``last_grain`` = (S16,
    r, C16, curve, seed) or None and ``last_grain_payloads`` = the payloads grained.  Without it no buffer, table, launch or stream is added
    and every byte stays the same.  ``lut``: None (default), the path of a ``.cube`` file or a ``lut3d.Cube``: a 3D colour LUT applied on the GPU to every
    payload written, between the scaler and the encode (``demfi_amd.lut3d``; csrc/lut3d.hip ``demfi_rgb_lut3d``, ONE launch per batch); the
    egress then runs on RGB payloads whether or not the run is in linear light.  A file that does not parse and a working depth above 12
    bits are refused, the latter at construction where ``work_depth`` says so and else once the header is known.  Any number of ranks.
    After a run ``last_lut`` = the cube or None and ``last_lut_payloads`` = the payloads taken through it.  ``deblock``: None (default), True (the thresholds 16:4), A (A : (A + 3) // 4), (A, B) or an "A[:B]" string,
    at the 8-bit scale with 0 <= B <= A <= 255: the block edges of every uploaded payload are smoothed in place on the GPU at the top of the
    ingest (``demfi_amd.deblock``, csrc/deblock.hip ``demfi_payload_deblock``, ONE launch per run of uploaded slots), on the grid of 8 of the
    uncropped stream (``crop`` gives the phases), field by field under ``deinterlace``; everything behind runs on the deblocked stream.  Goes
    with every other switch and any number of ranks.  ``deblock=0`` builds no stage.  After a run ``last_deblocked`` = the payloads
    deblocked.  Without it no buffer, table, launch or counter is added and every byte stays the same.  ``dering``: None (default), True (the
    strengths 4:2:5, AV1's middle of the range, not tuned against this network), P (P : min((P + 1) // 2, 4) : 5), (P, S), (P, S, D) or a
    "P[:S[:D]]" string, at the 8-bit scale with 0 <= P <= 15, 0 <= S <= 4, 3 <= D <= 6: ringing beside edges is smoothed on the GPU behind the
    deblocker (``demfi_amd.dering``: AV1's CDEF; csrc/dering.hip ``demfi_payload_dering``, one device copy into a scratch buffer and ONE launch
    per run of uploaded slots), on the block grid of the uncropped stream, field by field under ``deinterlace``; everything behind runs on the
    deringed stream.  Goes with every other switch and any number of ranks.  ``dering=(0, 0)`` builds no stage.  After a run ``last_deringed``
    = the payloads deringed.  Without it no buffer, table, launch, copy or counter is added and every byte stays the same.  ``deband``: None
    (default), True (2:16, not tuned against this network), T (T:16), (T, R) or a "T[:R]" string, T in 8-bit steps with 0 <= T <= 8, R in
    samples with 1 <= R <= 16: bands are smoothed on the GPU directly behind the deringing filter (``demfi_amd.deband``: a range-limited box
    mean; csrc/deband.hip ``demfi_payload_deband``, one device copy into a scratch buffer, shared with ``dering``, and ONE launch per run of
    uploaded slots), field by field under ``deinterlace``; everything behind runs on the debanded stream.  It does its work at a working
    depth above the input's (``work_depth=10`` or more on 8-bit input) and is not refused without.  Goes with every other switch and any
    number of ranks.  ``deband=0`` builds no stage.  After a run ``last_debanded`` = the payloads debanded.  Without it no buffer, table,
    launch, copy or counter is added and every byte stays the same.  ``nlmeans``: None (default), True (3:2:5, not tuned against this
    network), S (S:2:5), (S, P, R) or a "S[:P[:R]]" string, S in 8-bit steps with 0 <= S <= 16, P and R in samples with 1 <= P <= 3 and
    1 <= R <= 7: every plane is denoised within the frame on the GPU behind the deringing filter and in front of the debander
    (``demfi_amd.nlmeans``: non-local means in exact integers; csrc/nlmeans.hip ``demfi_payload_nlmeans``, one device copy into the scratch
    buffer ``dering`` and ``deband`` use and ONE launch per run of uploaded slots), field by field under ``deinterlace``; everything behind
    runs on the filtered stream.  Goes with every other switch and any number of ranks.  ``nlmeans=0`` builds no stage.  After a run
    ``last_nlm_filtered`` = the payloads filtered.  Without it no buffer, table, launch, copy or counter is added and every byte stays the
    same."""

    def __init__(self, model, n_tst=3, mfi=None, batch=4, matrix='auto', fps=None, scene_cut=None, full_length=False, tile=None,
                 tile_margin=T.DEFAULT_MARGIN, high_depth=False, layouts=False, dedup=None, dedup_max_hold=K.DEFAULT_MAX_HOLD,
                 tile_high_depth=False, deinterlace=False, deinterlace_mode='bob', ivtc=False, ivtc_cthresh=TC.DEFAULT_CTHRESH,
                 ivtc_combpel=TC.DEFAULT_COMBPEL, ivtc_combed=TC.DEFAULT_COMBED, crop=None, crop_limit=LB.DEFAULT_LIMIT,
                 crop_noise=LB.DEFAULT_NOISE, crop_probe=LB.DEFAULT_PROBE, crop_output='pad', shutter=None,
                 shutter_samples=None, interlace=None, interlace_lowpass=None, scale=None, scale_filter=None, work_depth=None,
                 out_depth=None, dither=None, down=False, shutter_window=None, denoise=None, denoise_radius=None, linear_light=None,
                 out_matrix=None, out_range=None, grain=None, grain_size=None, grain_chroma=None, grain_curve=None, grain_seed=None,
                 deblock=None, dering=None, deband=None, lut=None, nlmeans=None, **runner_kw):
        self.nlmeans = check_nlmeans(nlmeans)            # (S, P, R) or None
        check_deinterlace_mode(deinterlace, deinterlace_mode, dedup)
        self.lut = check_lut(lut)                        # a ``lut3d.Cube`` or None
        self.last_lut = None
        self.deblock = check_deblock(deblock)            # (A, B) or None
        self.dering = check_dering(dering)               # (P, S, D) or None
        self.deband = check_deband(deband)               # (T, R) or None
        self.grain = check_grain(grain, grain_size, grain_chroma, grain_curve, grain_seed)   # (S16, r, C16, curve, seed) or None
        self.last_grain = None
        self.colour = check_colour(linear_light, out_matrix, out_range, auto=True)   # (transfer, out matrix or 'auto', out full range) or None
        self.last_colour = None
        self.denoise = check_denoise(denoise, denoise_radius, dedup, deinterlace_mode)   # (A, B, R) or None
        self.down = bool(down)
        self.work_depth, self.out_depth, self.dither = check_depths(work_depth, out_depth, dither)
        check_lut(self.lut, self.work_depth)             # a working depth above 12 bits is refused here where the switch names it
        self.scale = check_scale(scale, scale_filter, crop, crop_output)  # (w, h, filter) or None
        self.interlace = check_interlace(interlace, interlace_lowpass)    # (order, low-pass mode) or None
        self.shutter = check_shutter(shutter, shutter_samples, dedup)     # (S, D) or None
        self.shutter_window = check_shutter_window(self.shutter, shutter_window)     # 'box' / 'triangle', None without a shutter
        self.last_depths = self.last_scale = self.last_interlace = self.last_shutter = self.last_shutter_window = None
        self.last_windows_skipped = 0
        for attr in filter(None, list(COUNTERS.values()) + list(INGEST_COUNTERS.values()) + list(EGRESS_COUNTERS.values())):
            setattr(self, attr, 0)
        self.crop, (self.crop_limit, self.crop_noise, self.crop_probe, self.crop_output) = check_crop(
            crop, crop_limit, crop_noise, crop_probe, crop_output)
        self.last_crop, self.last_crop_probed, self.last_crop_note, self.last_crop_seconds = None, 0, None, 0.0
        self.last_input_size = None
        self.ivtc = bool(ivtc)
        self.ivtc_params = TC.check_params(ivtc_cthresh, ivtc_combpel, ivtc_combed)
        check_ivtc(self.ivtc, deinterlace)
        self._film = None
        self._matrix_h = None                            # a cropped run: the input's own height chooses the 'auto' matrix
        self.deinterlace_mode = deinterlace_mode
        if matrix not in ('auto',) + tuple(y4m.MATRICES):
            raise ValueError("matrix must be 'auto', 'bt601' or 'bt709', got %r" % matrix)
        if mfi is not None and fps is not None:
            raise ValueError('VideoRunner: give mfi or fps, not both')
        if fps is not None and not isinstance(fps, (str, int, Fraction)) or isinstance(fps, bool):
            raise TypeError('VideoRunner: fps must be a Fraction, an int or an "N/D" string (a float is not exact: 59.94 is not '
                            '60000/1001), got %r' % (fps,))
        self.fps = R.parse_fps(fps) if isinstance(fps, str) else (Fraction(fps) if fps is not None else None)
        if self.fps is not None and self.fps <= 0:
            raise ValueError('VideoRunner: fps must be > 0, got %s' % self.fps)
        mfi = 8 if mfi is None and fps is None else mfi
        self.model, self.n_tst, self.mfi, self.batch, self.matrix = model, n_tst, mfi, batch, matrix
        self.scene_cut = S.check_threshold(scene_cut) if scene_cut is not None else None
        self.full_length = bool(full_length)
        self.high_depth = bool(high_depth)
        self.tile_high_depth = bool(tile_high_depth)
        self.deinterlace = bool(deinterlace)
        self.last_fields = None
        self.depths = y4m.DEPTHS if self.high_depth else (8,)
        self.layouts = y4m.LAYOUTS if layouts else ('420',)
        self.tile = tile
        self.last_depth, self.last_layout = 8, '420'
        if tile is not None:
            T.plan_tiles(64, 64, tile, tile_margin)      # a bad tile or margin fails here, not at the first frame
        self.runner_kw = dict(runner_kw, tile=tile, tile_margin=tile_margin)
        self.last_plan = None
        self._runners = {}
        self.last_decode_peak = 0
        self.last_instants = (0, 0)
        self.last_st_frames = 0
        self.last_fps_out = None
        self.last_cuts = []
        if dedup is None or dedup is False:
            self.dedup = None
            K.check_params(max_hold=dedup_max_hold)
        else:
            self.dedup = K.check_params(*(K.DEFAULTS if dedup is True else tuple(dedup)), max_hold=dedup_max_hold)
        self.last_dups = []

    def _ratio(self, hdr):
        """The ratio r = F_out / F_in of this input: M for x M, whose per-window plans (``retime``) give exactly the x M stream."""
        return Fraction(self.mfi) if self.mfi is not None else R.ratio(hdr.fps, self.fps, self.down)

    def _scale_of(self, hdr):
        """What the scale stage does to a run on frames of ``hdr``: None (no switch, or the run's own size: no stage), or (w, h, filter).
        Before anything is allocated: with interlaced output h lies on the interlaced grid, and no plane takes more than 32 taps."""
        if self.scale is None:
            return None
        w, h, filt = self.scale
        if self.interlace is not None:
            SC.check_interlaced_rows(h, hdr.layout)
        if (w, h) == (hdr.w, hdr.h):
            return None
        for (ri, ci), (ro, co) in zip(IL.plane_shapes(hdr.h, hdr.w, hdr.layout), IL.plane_shapes(h, w, hdr.layout)):
            for n_in, n_out in ((ci, co), (ri, ro)):
                if SC.n_taps(n_in, n_out, filt) > SC.MAX_TAPS:
                    SC.axis_table(n_in, n_out, filt)                     # the refusal, in its own words
        return self.scale

    def _depths_of(self, hdr):
        """(input, working, output depth, dither mode or None) of a run on the stream of ``hdr`` (``bitdepth.resolve``, with its refusals),
        before anything is allocated; without the switches three times the input's depth."""
        return BD.resolve(hdr.depth, self.work_depth, self.out_depth, self.dither)

    def _out_header(self, hdr):
        ohdr = BD.depth_header(R.output_header(hdr, hdr.fps * self._ratio(hdr)), self._depths_of(hdr)[2])
        sc = self._scale_of(hdr)
        if sc is not None:                           # the size and the pixel aspect that keeps the display aspect
            ohdr = SC.scaled_header(ohdr, sc[0], sc[1])
        if self.interlace is not None:               # the same stream as fields: the I tag of the order, half the rate
            ohdr = IL.interlaced_header(ohdr, self.interlace[0])
        if self.colour is not None:                  # the range written; Y4M has no tag for the matrix
            ohdr = CL.range_header(ohdr, self._colour_of(hdr)[2])
        self.last_fps_out = ohdr.fps
        return ohdr

    def _in_matrix(self, hdr):
        """The matrix of the input: ``matrix``, 'auto' by the input's own height (a cropped run: the full frame's)."""
        return y4m.auto_matrix(self._matrix_h or hdr.h) if self.matrix == 'auto' else self.matrix

    def _colour_of(self, hdr):
        """(transfer or None, matrix, full range) the run on frames of ``hdr`` writes with, or None without the colour switches;
        ``colour.resolve``: 'auto' goes by the height actually written -- behind the scaler, and with ``crop_output`` 'pad' the full
        frame's.  Before anything is allocated: linear light at a working depth above 12 bits is refused."""
        if self.colour is None:
            return None
        transfer, matrix, full = self.colour
        if transfer is not None:
            CL.check_depth(self._depths_of(hdr)[1])
        sc = self._scale_of(hdr)
        out_h = sc[1] if sc is not None else (self._matrix_h or hdr.h) if self.crop_output == 'pad' else hdr.h
        matrix, full = CL.resolve(matrix, None if full is None else 'full' if full else 'limited', self._in_matrix(hdr), hdr.full_range, out_h)
        return transfer, matrix, full

    def _n_out(self, n_in, hdr):
        """Payloads written for n_in input frames: the output frames, or with ``interlace`` their pairs."""
        n = R.n_output_frames(n_in, self._ratio(hdr), self.full_length)
        return IL.n_payloads(n) if self.interlace is not None else n

    def _progressive(self, hdr):
        """(the header everything downstream works on, field order or None, input frames per payload) of an input with header
        ``hdr``: an interlaced stream counts as its fields, a progressive stream at twice the rate (``deint.progressive_header``).
        Before anything is allocated: a requested output rate below the field rate is refused here."""
        if self.ivtc:
            fhdr = TC.film_header(hdr)
            self.last_fields = None
            if self.fps is not None and self.fps < fhdr.fps and not self.down:
                raise ValueError('VideoRunner: output frame rate %s is below the film rate %s of the telecined input (%s frames/s, four '
                                 'film frames in five): --ivtc gives the film frames, so F_out must be at least %s (or pass --downconvert)'
                                 % (self.fps, fhdr.fps, hdr.fps, fhdr.fps))
            return fhdr, None, 1
        order = hdr.interlace if hdr.interlace in ('t', 'b') else None
        self.last_fields = {'t': 'tff', 'b': 'bff', None: None}[order]
        if order is None:
            return hdr, None, 1
        phdr = I.progressive_header(hdr)
        if self.fps is not None and self.fps < phdr.fps and not self.down:
            raise ValueError('VideoRunner: output frame rate %s is below the field rate %s of the interlaced input (%s frames/s, two fields '
                             'each): --deinterlace gives one frame per field, so F_out must be at least %s (or pass --downconvert)'
                             % (self.fps, phdr.fps, hdr.fps, phdr.fps))
        return phdr, order, 2

    @property
    def last_matches(self):
        return self._film.matches if self._film is not None else {c: 0 for c in TC.CANDIDATES}

    @property
    def last_dropped(self):
        return self._film.dropped if self._film is not None else []

    @property
    def last_combed(self):
        return list(self._film.combed) if self._film is not None else []

    def _film_frames(self, read, hdr, device):
        """``telecine.FilmFrames`` over the input payloads ``read`` gives (``hdr``: the input's header), scored on the GPU."""
        from .y4m_edge import IvtcScorer
        cthresh, combpel, combed = self.ivtc_params
        self._film = TC.FilmFrames(read, hdr, IvtcScorer(L.load(), hdr.h, hdr.w, hdr.depth, cthresh, device), combpel, combed)
        return self._film

    def _crop_stage(self, in_hdr, per, probe=None):
        """The ``letterbox.Cropper`` of this input (``in_hdr``: its header, ``per``: 2 when its payloads stay interlaced), or None
        when nothing is cropped; before anything else is allocated for the input.  ``probe()``: the pre-pass of 'auto', which gives the
        detected rectangle or None.  Sets ``last_crop`` (the rectangle or None), ``last_crop_probed`` and ``last_crop_note``."""
        self.last_crop, self.last_crop_probed, self.last_crop_note, self.last_crop_seconds = None, 0, None, 0.0
        self.last_input_size = (in_hdr.h, in_hdr.w)
        if self.crop is None:
            return None
        if self.crop == 'auto':
            rect, explicit = probe(), False
        else:
            rect, explicit = LB.bars_rect(self.crop, in_hdr.h, in_hdr.w), True
        # interlaced output: the rectangle must keep field parity in every plane of the written payloads, as for interlaced input
        self.last_crop, self.last_crop_note = LB.check_rect(rect, in_hdr.h, in_hdr.w, in_hdr.layout, 2 if self.interlace is not None else per,
                                                            explicit)
        return LB.Cropper(in_hdr, self.last_crop) if self.last_crop is not None else None

    def crop_report(self):
        """One line on what the crop stage of the last run did."""
        if self.last_crop is None:
            line = self.last_crop_note or 'crop: the picture fills the frame; nothing is cropped'
        else:
            (t, b, l, r), (h, w) = self.last_crop, self.last_input_size
            line = 'crop: bars %d:%d:%d:%d (T:B:L:R), %dx%d of %dx%d runs, output %s' % (t, h - b, l, w - r, r - l, b - t, w, h,
                                                                                          self.crop_output)
        if self.crop == 'auto':
            line += '; %d payloads probed in %.2f s' % (self.last_crop_probed, self.last_crop_seconds)
        return line

    def _probe_rect(self, f, offs, in_hdr):
        """The pre-pass of ``crop='auto'`` over the scanned file ``f``: the union of the extents of the probed payloads' luma planes,
        counted on the GPU.  Every rank probes the same payloads and arrives at the same rectangle: no collective."""
        import time
        from .y4m_edge import LineScorer
        t0 = time.perf_counter()
        sc = LineScorer(L.load(), in_hdr.h, in_hdr.w, in_hdr.depth, self.crop_limit, next(self.model.parameters()).device)
        ext = LB.Extent(self.crop_noise)
        for rows, cols in sc.counts(f, offs, LB.probe_indices(len(offs), self.crop_probe)):
            ext.push(rows, cols)
        self.last_crop_probed, self.last_crop_seconds = sc.probed, time.perf_counter() - t0
        return ext.rect()

    def _headers(self, full_hdr, cropper):
        """(the header everything downstream works on, the header of the output written) of an input whose progressive header is
        ``full_hdr``: the cropped one runs; the full size is written unless ``crop_output`` is 'cropped'."""
        if cropper is None:
            return full_hdr, self._out_header(full_hdr)
        hdr = LB.cropped_header(full_hdr, cropper.rect)
        ohdr = self._out_header(hdr)
        return hdr, (ohdr if self.crop_output == 'cropped' else LB.resized_header(ohdr, full_hdr.h, full_hdr.w))

    @staticmethod
    def _cropped(fetch, cropper):
        """``fetch(i, buf)`` of full payloads -> one of cropped payloads: the full payload goes into a scratch buffer, its rectangle into ``buf``."""
        if cropper is None:
            return fetch
        import numpy as np
        scratch = np.empty(cropper.Pf, np.uint8)

        def crop_fetch(i, buf):
            if not fetch(i, scratch):
                return False
            cropper.crop_into(scratch, buf)
            return True
        return crop_fetch

    def _padded(self, sink, cropper):
        """``sink(k, payloads)`` of full payloads -> one of cropped payloads, padded back to the full size with black on the way."""
        if cropper is None or self.crop_output == 'cropped':
            return sink
        import numpy as np
        out = self._depths_of(cropper.full)[2]
        if out != cropper.full.depth:                # the payloads written have the output's depth: so have the bars and their black
            cropper = LB.Cropper(BD.depth_header(cropper.full, out), cropper.rect)
        if self.colour is not None:                  # and the range written: its black
            full = cropper.full.full_range if self.colour[2] is None else self.colour[2]
            if full != cropper.full.full_range:
                cropper = LB.Cropper(CL.range_header(cropper.full, full), cropper.rect)

        def pad_sink(k, payloads):
            full = np.empty((len(payloads), cropper.Pf), np.uint8)
            cropper.pad_into(payloads, full)
            sink(k, full)
        return pad_sink

    def _behind(self, order):
        """``y4m.Frames(behind=...)``: the reach of the edge's ingest.  The adaptive mode reads two fields before and after every field it
        rebuilds, the denoiser R frames (over the fields of an interlaced input 2 R)."""
        if self.denoise is not None:
            return DN.reach(self.denoise[2], order is not None)
        return 2 if order is not None and self.deinterlace_mode == 'adaptive' else 0

    def _check_depth(self, hdr):
        """Before anything is allocated for this input: the depths resolve (``_depths_of``), and frames above 8 bits -- the WORKING depth
        decides -- run as tiles only with ``tile_high_depth``.  ``last_depth`` is the depth written."""
        d_in, work, out, _ = depths = self._depths_of(hdr)
        if work > 8 and self.tile is not None and not self.tile_high_depth:
            what = 'a %d-bit stream (C%s)' % (hdr.depth, hdr.ctag) if work == d_in else 'a working depth of %d bits (--work-depth / --out-depth)' % work
            raise ValueError('VideoRunner: tile=%r with %s: tiles move 8-bit pixels, so --tile and high bit '
                             'depth do not go together unless asked for; run it untiled, %s, or pass '
                             '--tile-high-depth (tile_high_depth=True)' % (self.tile, what, 'convert the input to 8 bits' if work == d_in
                                                                           else 'work at 8 bits'))
        self._colour_of(hdr)                         # linear light above 12 bits is refused here
        check_lut(self.lut, work)                    # and so is a LUT
        self.last_depths = None if BD.is_noop(depths) else depths
        self.last_depth, self.last_layout = out, hdr.layout

    def _fine_ratio(self, hdr):
        """The ratio the runner is built with: r, or with a shutter that of the fine stream, r D (refused above ``retime.MAX_RATIO``).
        ``dedup`` is refused here for r < 1: ``cadence`` plans over the kept frames for r >= 1 only."""
        r = self._ratio(hdr)
        if r < 1 and self.dedup is not None:
            raise ValueError('VideoRunner: --dedup does not go with an output rate below the input\'s (%s of it, --downconvert): repeated '
                             'frames are planned for F_out >= F_in only; run one of the two' % r)
        return r if self.shutter is None else SH.fine_ratio(r, self.shutter[1])

    def _clip_runner(self, hdr, world, rank):
        r, kw = self._fine_ratio(hdr), {}
        key = (hdr.h, hdr.w, world, rank, r, self.shutter)   # the window is the edge's (``EdgeSpec``), not the runner's
        cr = self._runners.get(key)
        if cr is None:
            if self.shutter is not None:             # only some of the fine ratio's instants run: the batched plan is sized by those
                kw['instant_counts'] = SH.period_counts(self._ratio(hdr), *self.shutter)
            cr = self._runners[key] = ClipRunner(self.model, hdr.h, hdr.w, self.n_tst, self.mfi or 8, batch=self.batch, world=world,
                                                 rank=rank, **dict(self.runner_kw, retime=r, **kw))
        self.last_plan = cr.plan
        return cr

    def _run(self, cr, hdr, first, fn):
        """fn() runs windows lo, lo+1, ... of the input on cr, lo = first() once it has run; returns its window count and sets
        the per-run counters."""
        rn = cr.runner
        before, skipped = {name: getattr(rn, name) for name in (*COUNTERS, *INGEST_COUNTERS, *EGRESS_COUNTERS)}, rn.windows_skipped
        with cr.oversize_hint():
            n = fn()
        lo, r = first(), self._ratio(hdr)
        self.last_windows_skipped = rn.windows_skipped - skipped
        self._counted(hdr, {name: getattr(rn, name) - before[name] for name in before}, list(rn.last_cuts) if self.scene_cut is not None else [],
                      sum(kind == R.ST for k in range(lo, lo + n) for _, kind, _ in R.window_outputs(k, r, full_length=self.full_length)))
        return n

    def _counted(self, hdr, added, cuts, st_frames):
        """The per-run values of a run on the stream of ``hdr``: ``added[name]`` is what it added to the runner's counter ``name`` of
        ``COUNTERS`` (a rank without a window: zeros), ``cuts`` the frames that start a scene, ``st_frames`` the St frames its windows own."""
        for name, attr in COUNTERS.items():
            if attr is not None:
                setattr(self, attr, added[name])
        for name, attr in (*INGEST_COUNTERS.items(), *EGRESS_COUNTERS.items()):
            setattr(self, attr, added.get(name, 0))
        self.last_colour = self._colour_of(hdr)
        self.last_instants, self.last_cuts = (added['instants_run'], added['instants_padded']), cuts
        self.last_st_frames = added['shutter_mixed'] if self.shutter is not None else st_frames     # the fine frames that went into the mixes
        self.last_shutter, self.last_scale, self.last_shutter_window = self.shutter, self._scale_of(hdr), self.shutter_window
        self.last_interlace, self.last_grain = self.interlace[0] if self.interlace is not None else None, self.grain
        self.last_lut = self.lut

    def _edge(self, hdr, with_s1, order=None):
        depths = self._depths_of(hdr)                # hdr has the input's depth; the edge works at depths[1]
        colour = self._colour_of(hdr)
        kw = {} if colour is None else {'linear_light': colour[0], 'out_matrix': colour[1], 'out_range': 'full' if colour[2] else 'limited'}
        return YuvEdge(self._in_matrix(hdr), hdr.full_range, hdr.chroma, with_s1,
                       self.scene_cut, self.full_length, depths[1], hdr.layout, self.dedup, order, self.deinterlace_mode, self.shutter,
                       *(self.interlace or (None, None)), self._scale_of(hdr), depths=depths, shutter_window=self.shutter_window,
                       denoise=self.denoise, grain=self.grain, deblock=self.deblock, dering=self.dering, deband=self.deband, lut=self.lut,
                       nlmeans=self.nlmeans,
                       crop_rect=self.last_crop if self.deblock is not None or self.dering is not None else None, **kw)

    def _run_dedup(self, cr, hdr, frames, sink, order=None):
        """The --dedup run of ``frames`` (``y4m.Frames`` over the whole input) on cr: the windows are those of the kept frames."""
        det = K.Detector(hdr.h, hdr.w, *self.dedup)
        kf = KeptFrames(frames, det, self._ratio(hdr), self.full_length)
        n = self._run(cr, hdr, lambda: 0, lambda: cr.runner.run_clip_u8(kf, kf.windows(), sink, batch=self.batch,
                                                                       yuv=self._edge(hdr, lambda j: False, order), window_index=kf.index))
        self.last_st_frames, self.last_dups = kf.st_frames, list(det.dups)
        self.last_cuts = [det.kept[j] for j in self.last_cuts]      # scored over the kept sequence: back to input frames
        self.last_decode_peak = frames.peak
        return n

    def run_stream(self, src, dst):
        """One rank, sequential binary streams (stdin / stdout work): nothing is seeked, the input is read in batches of
        windows and every batch is written (and flushed) as it drains.  Returns (windows, frames written)."""
        if self.crop == 'auto':
            raise ValueError('VideoRunner.run_stream: ' + AUTO_NEEDS_A_FILE)
        rd = y4m.Reader(src, self.depths, self.layouts, self.deinterlace, self.ivtc)
        self._film = None
        full_hdr, order, per = self._progressive(rd.header)
        cropper = self._crop_stage(rd.header, per)
        hdr, out_hdr = self._headers(full_hdr, cropper)  # hdr: what runs (cropped); out_hdr: what is written
        self._matrix_h = full_hdr.h if cropper is not None else None
        self._check_depth(hdr)
        self._fine_ratio(hdr)
        cr = self._clip_runner(hdr, 1, 0)
        wr = y4m.Writer(dst, out_hdr)
        if self.ivtc:                                    # downstream sees an ordinary progressive input at the film rate
            film = self._film_frames(lambda i, buf: rd.read_into(buf), rd.header, cr.runner.engine.device)
            frames = y4m.Frames(payload=hdr.payload, fetch=self._cropped(film, cropper), full_length=self.full_length,
                                behind=self._behind(None))
        elif cropper is not None:                        # the crop is the last host stage in front of the frames
            frames = y4m.Frames(payload=hdr.payload, fetch=self._cropped(lambda i, buf: rd.read_into(buf), cropper),
                                full_length=self.full_length, fields=per, behind=self._behind(order))
        else:
            frames = y4m.Frames(rd, full_length=self.full_length, fields=per, behind=self._behind(order))
        self.last_dups = []

        def write(k, payloads):
            wr.write(payloads)
            dst.flush()
        sink = self._padded(write, cropper)
        if self.dedup is not None:
            n = self._run_dedup(cr, hdr, frames, sink, order)
            dst.flush()
            return n, wr.frames
        if self.full_length:                             # window j of the sequence is window first_window + j
            def index(j):
                return frames.first_window + j
            edge, kw = self._edge(hdr, lambda j: frames.is_last(index(j)), order), {'window_index': index}
        else:
            edge, kw = self._edge(hdr, frames.is_last, order), {}
        n = self._run(cr, hdr, lambda: frames.first_window or 0,
                      lambda: cr.runner.run_clip_u8(frames, frames.windows(), sink, batch=self.batch, yuv=edge, **kw))
        dst.flush()
        self.last_decode_peak = frames.peak
        return n, wr.frames

    def run_file(self, in_path, out_path, world=1, rank=0):
        """Rank ``rank`` of ``world`` on regular files: one scan of the input's frame headers, this rank's block of windows
        (``dist.shard_windows``), its frames written at ``header + i*(6 + payload)``.  Rank 0 writes the header and sizes the
        output file; all ranks meet at a barrier before writing.  Returns (windows, frames written) of this rank."""
        check_one_rank(world, dedup=self.dedup, ivtc=self.ivtc, shutter=self.shutter, interlace=self.interlace, grain=self.grain)
        self.last_dups, self._film = [], None
        with open(in_path, 'rb') as f:
            in_hdr, _, offs = y4m.scan(f, self.depths, self.layouts, self.deinterlace, self.ivtc)
            full_hdr, order, per = self._progressive(in_hdr)
            cropper = self._crop_stage(in_hdr, per, lambda: self._probe_rect(f, offs, in_hdr))
            hdr, out_hdr = self._headers(full_hdr, cropper)                          # hdr: what runs (cropped); out_hdr: what is written
            self._matrix_h = full_hdr.h if cropper is not None else None
            self._check_depth(hdr)
            self._fine_ratio(hdr)
            n_in = TC.n_film_frames(len(offs)) if self.ivtc else per * len(offs)     # an interlaced input counts as its fields
            hb = out_hdr.encode()
            total = self._n_out(n_in, hdr)
            if rank == 0:
                with open(out_path, 'wb') as o:
                    o.write(hb)
                    o.truncate(y4m.frame_offset(len(hb), total, out_hdr.payload))
            D.barrier()
            cr = self._clip_runner(hdr, world, rank)
            full = self.full_length

            def file_frames(first, stop, **kw):
                """Frames first .. stop-1 of the input: its payloads by seek, or (one rank, from frame 0) the film frames made of them."""
                if not self.ivtc and cropper is None:
                    return y4m.Frames.from_file(f, offs, first, stop, hdr.payload, **kw)
                if not self.ivtc:                        # ``from_file`` with the crop behind its fetch
                    return y4m.Frames(payload=hdr.payload, fetch=self._cropped(y4m.file_fetch(f, offs), cropper), first=first,
                                      stop=min(stop + kw.get('behind', 0), kw.get('fields', 1) * len(offs)), **kw)
                if first != 0:
                    raise RuntimeError('ivtc: film frames are made in order from frame 0, not from frame %d' % first)
                fetch = y4m.file_fetch(f, offs)
                film = self._film_frames(lambda i, buf: i < len(offs) and fetch(i, buf), in_hdr, cr.runner.engine.device)
                return y4m.Frames(payload=hdr.payload, fetch=self._cropped(film, cropper), stop=min(stop + kw.get('behind', 0), n_in),
                                  behind=kw.get('behind', 0))
            if self.dedup is not None:
                with open(out_path, 'r+b') as o:
                    wr = y4m.Writer(o, out_hdr, at=len(hb))
                    n = self._run_dedup(cr, hdr, file_frames(0, n_in, fields=per), self._padded(lambda k, p: wr.write(p), cropper), order)
                return n, wr.frames
            lo, wins = cr.my_windows(n_in, full)
            if not wins:
                self._counted(hdr, dict.fromkeys(COUNTERS, 0), [], 0)
                self.last_windows_skipped = 0
                return 0, 0
            last = R.first_window(n_in, full) + R.n_windows(n_in, full) - 1
            # scene cuts: a block starting at window lo >= 1 also reads frame lo - 1 (score_{lo+1} needs mafd_lo)
            first = S.first_frame(lo) if self.scene_cut is not None else max(lo, 0)
            frames = file_frames(first, lo + len(wins) + 3, fields=per, behind=self._behind(order))
            # interlaced output is one rank's: its payloads follow the header
            at = len(hb) if self.interlace is not None else R.block_offset(len(hb), lo, self._ratio(hdr), out_hdr.payload, full)
            kw = {'window_index': lambda j: lo + j} if full else {}
            with open(out_path, 'r+b') as o:
                wr = y4m.Writer(o, out_hdr, at=at)
                sink = self._padded(lambda k, p: wr.write(p), cropper)
                n = self._run(cr, hdr, lambda: lo, lambda: cr.runner.run_clip_u8(frames, wins, sink, batch=self.batch,
                                                                                 yuv=self._edge(hdr, lambda k: lo + k == last, order), **kw))
            self.last_decode_peak = frames.peak
            return n, wr.frames


def _is_regular(path):
    return path != '-' and (not os.path.exists(path) or os.path.isfile(path))


def _value_arg(fn):
    def arg(text):
        try:
            return fn(text)
        except ValueError as e:
            import argparse
            raise argparse.ArgumentTypeError(str(e))
    return arg


def _grain_arg(fn):
    """The text of a decimal grain switch, checked by ``fn`` and handed on as it is: ``VideoRunner`` takes S and C, not their sixteenths."""
    def arg(text):
        fn(text)
        return text.strip()
    return arg


_crop_arg = _value_arg(LB.parse_crop)
_crop_probe_arg = _value_arg(LB.parse_probe)
_crop_noise_arg = _value_arg(lambda text: LB.check_params(noise=text.replace(':', '/'))[1])


def parser():
    """The command line of ``main``."""
    import argparse
    ap = argparse.ArgumentParser(prog='python -m demfi_amd.video', description=main.__doc__.split('\n\n')[0],
                                 epilog='Input: 8-bit 4:2:0 progressive Y4M (Ip, I? or no I tag; C420jpeg, C420, C420mpeg2; XCOLORRANGE=FULL|LIMITED), '
                                        'e.g. ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe -; with --high-depth also 10- to 16-bit '
                                        '4:2:0 (C420p10, C420p12, C420p14, C420p16), e.g. ffmpeg -i in.mkv -pix_fmt yuv420p10le -strict -1 '
                                        '-f yuv4mpegpipe -; with --any-layout also 4:2:2, 4:4:4 and grey (C422, C444, Cmono and, with '
                                        '--high-depth, C422pNN, C444pNN, CmonoNN), e.g. ffmpeg -i in.mov -pix_fmt yuv422p10le -strict -1 '
                                        '-f yuv4mpegpipe -; with --deinterlace also interlaced streams of a fixed field order (It, Ib), every '
                                        'field a frame at twice the rate.  Output: progressive (with --interlace: It or Ib at half the rate), the input\'s size (with --scale: WxH), C420jpeg (C420pNN at the input\'s depth; the input\'s layout and '
                                        'depth for the other layouts; with --out-depth D, or --work-depth W alone, the tag of depth D, or of the input\'s), the input\'s '
                                        'matrix and range.  n input frames give (n-3)*M + 1 output frames: the first and the last '
                                        'input frame have no output, as in the reference (--full-length: n*M frames from input '
                                        'frame 0 on).  All logging goes to stderr.')
    ap.add_argument('input', help="Y4M file, or - for stdin")
    ap.add_argument('output', help="Y4M file, or - for stdout")
    rate = ap.add_mutually_exclusive_group()
    rate.add_argument('--mfi', type=int, default=None, help='multiple_MFI: output frame rate = M x input (main.py:98); default 8')
    rate.add_argument('--fps', type=_value_arg(R.parse_fps), default=None,
                      help='output frame rate N, N/D or N:D (exact: 60000/1001, not 59.94), at least the input rate (below it with '
                           '--downconvert); output frame i is at input time 1 + i*F_in/F_out')
    ap.add_argument('--downconvert', action='store_true',
                    help='let --fps lie below the input rate (down to 1/%d of it; behind --deinterlace below the field rate, behind --ivtc '
                         'below the film rate): 60p -> 25p, 59.94i -> 50i with --deinterlace --fps 50 --interlace tff.  The output frames '
                         'sit on the same timeline, further apart; windows that own no output frame run nothing.  Use --shutter with it: '
                         'the temporal aperture is what keeps a lower rate from juddering.  Not with --dedup.  Changes nothing for '
                         'F_out >= F_in.  Off by default (a lower rate is refused)' % R.MAX_RATIO)
    ap.add_argument('--n-tst', type=int, default=3, help='N_tst recursive boosts (main.py:101)')
    ap.add_argument('--dtype', default='fp16', choices=['fp16', 'fp32'])
    ap.add_argument('--checkpoint', default='', help="reference checkpoint (.pt holding 'state_dict_Model')")
    ap.add_argument('--matrix', default='auto', choices=['auto', 'bt601', 'bt709'],
                    help='YCbCr matrix of the input (and output); auto: BT.709 when H >= 720, else BT.601')
    ap.add_argument('--batch', type=int, default=4, help='windows per batch (the input frames held are bounded by it)')
    ap.add_argument('--scene-cut', nargs='?', type=_value_arg(S.check_threshold), const=S.DEFAULT_THRESHOLD, default=None, metavar='T',
                    help='detect scene cuts (score = min(mafd, |mafd - previous mafd|) of the payload samples, in percent; a cut where '
                         'score >= T, T in (0, 100], default %g) and never interpolate across one: the frames next to a cut '
                         'hold the nearest input frame.  Off unless given' % S.DEFAULT_THRESHOLD)
    ap.add_argument('--full-length', action='store_true',
                    help='cover the input\'s whole timeline: output frame 0 is input frame 0 and n input frames give ceil(n*F_out/F_in) '
                         'output frames (n*M with --mfi), the last input frame held to the end, so the video stays aligned with its '
                         'audio.  Off by default (the reference\'s timeline)')
    ap.add_argument('--high-depth', action='store_true',
                    help='also take 10-, 12-, 14- and 16-bit 4:2:0 (C420p10 .. C420p16, 16-bit little-endian samples) and write the '
                         'output at the input\'s depth, through a 16-bit frame path; --dtype fp16 resolves 10 bits fully and about 12 at '
                         'best, --dtype fp32 all 16.  With --tile only together with --tile-high-depth.  Off by default (8-bit input only)')
    ap.add_argument('--tile-high-depth', action='store_true',
                    help='let a 10- to 16-bit stream (--high-depth) run as tiles (--tile): every tile is read out of the full 16-bit '
                         'frames and its kept part written into the full output frames in place.  Changes nothing without both '
                         '--tile and --high-depth.  Off by default (such a stream is refused)')
    ap.add_argument('--any-layout', action='store_true',
                    help='also take 4:2:2, 4:4:4 and grey input (C422, C444, Cmono; together with --high-depth their 10- to 16-bit forms '
                         'C422pNN, C444pNN, CmonoNN) and write the output in the input\'s layout: nothing is resampled to 4:2:0 and back.  '
                         'Off by default (4:2:0 input only)')
    ap.add_argument('--dedup', action='store_true',
                    help='detect input frames that repeat the one before them (animation on twos and threes, 24p in a 30p or 60p '
                         'container, captures with dropped frames) and interpolate over them: a frame is a repeat when no 8x8 luma '
                         'block differs from the last kept frame by more than %d and at most %s of them by more than %d (the '
                         'defaults of ffmpeg\'s mpdecimate).  The output keeps its length and timing.  One rank only.  Off by '
                         'default' % (K.DEFAULT_HI, K.DEFAULT_FRAC, K.DEFAULT_LO))
    ap.add_argument('--deinterlace', action='store_true',
                    help='also take interlaced input (It: top field first, Ib: bottom field first; 1080i, 576i, 480i, DV) and bob it on '
                         'the GPU: every field becomes a progressive frame at its own time instant (the other field\'s rows are rebuilt '
                         'by an edge-directed line average), so n payloads at F count as 2n frames at 2F: --mfi M gives 2*M*F, --fps '
                         'must be at least 2F, and 50i --mfi 2 is 100p.  The output is progressive (fields again with --interlace).  Mixed-mode streams (Im) stay '
                         'refused (film carried by 3:2 pulldown: --ivtc).  Off by default (progressive input only); changes nothing for a progressive stream')
    ap.add_argument('--deinterlace-mode', default='bob', choices=list(I.MODES),
                    help='with --deinterlace: bob (default) rebuilds the other field\'s rows from the field alone; adaptive also looks at '
                         'the two fields before and the two after (yadif\'s temporal rule around the bob\'s value): static parts keep '
                         'their full vertical resolution and do not flicker, moving parts and scene cuts get the bob\'s value.  Costs '
                         'two fields of lookahead.  An error without --deinterlace, and with --dedup (use bob there)')
    ap.add_argument('--dedup-max-hold', type=int, default=K.DEFAULT_MAX_HOLD, metavar='N',
                    help='with --dedup: after N repeats in a row the next frame is kept whatever it shows (default %d), so a still '
                         'scene stays a sequence of frames N + 1 apart' % K.DEFAULT_MAX_HOLD)
    ap.add_argument('--ivtc', action='store_true',
                    help='inverse telecine: take film carried by 3:2 pulldown (24p as 29.97 frames/s; It, Ib, Im or a wrongly flagged Ip) '
                         'and put the film frames back together before anything else runs, as ffmpeg\'s fieldmatch,decimate does: every '
                         'payload keeps its top field and takes the bottom field that weaves to the least combed frame, and one frame '
                         'in five, the closest repeat, is dropped.  n payloads at F count as n - n//5 frames at 4F/5, so --fps must be at '
                         'least 4F/5 and --ivtc --fps 60000/1001 is the true 23.976 -> 59.94.  One rank only; not with --deinterlace.  '
                         'Off by default')
    ap.add_argument('--ivtc-cthresh', type=int, default=TC.DEFAULT_CTHRESH, metavar='T',
                    help='with --ivtc: the comb threshold in 8-bit steps, 0..255 (default %d, that of ffmpeg\'s fieldmatch): a sample is '
                         'combed when it differs from both rows next to it, in the same direction, by more than T' % TC.DEFAULT_CTHRESH)
    ap.add_argument('--ivtc-combpel', type=int, default=TC.DEFAULT_COMBPEL, metavar='N',
                    help='with --ivtc: a matched frame with more than N combed samples in one 16x16 luma block counts as combed '
                         '(default %d, ffmpeg\'s)' % TC.DEFAULT_COMBPEL)
    ap.add_argument('--ivtc-combed', default=TC.DEFAULT_COMBED, choices=list(TC.COMBED_MODES),
                    help='with --ivtc: what a matched frame that is still combed becomes (video inserts, bad edits, a stream that starts '
                         'mid-cycle): bob (default) rebuilds it from its top field, keep passes it through.  Its index is reported '
                         'either way')
    ap.add_argument('--crop', type=_crop_arg, default=None, metavar='auto|T:B:L:R',
                    help='keep letterbox and pillarbox bars away from the network: crop every payload to the picture, run on the smaller '
                         'frame, and pad the output back with black.  auto: find the bars in a pre-pass over the input (a regular file, '
                         'not a pipe); T:B:L:R: the widths of the top, bottom, left and right bars in luma samples, for instance from '
                         'ffmpeg -vf cropdetect (works on pipes).  Edges lie on the chroma grid (even for 4:2:0; rows in units of 4 with '
                         '--deinterlace); at least %dx%d is kept.  Off by default' % (LB.MIN_ACTIVE, LB.MIN_ACTIVE))
    ap.add_argument('--crop-limit', type=int, default=None, metavar='L',
                    help='with --crop auto: a luma sample above L (8-bit steps, 0..255) is lit; default %d, ffmpeg cropdetect\'s' % LB.DEFAULT_LIMIT)
    ap.add_argument('--crop-noise', type=_crop_noise_arg, default=None, metavar='N/D',
                    help='with --crop auto: a row or column is picture when more than this fraction of its samples is lit (default %s), '
                         'so specks do not make a line and subtitle text does' % LB.DEFAULT_NOISE)
    ap.add_argument('--crop-probe', type=_crop_probe_arg, default=None, metavar='all|N',
                    help='with --crop auto: look at all payloads (default) or at N spread evenly over the input')
    ap.add_argument('--crop-output', default=None, choices=list(LB.OUTPUTS),
                    help='with --crop: pad (default) writes the input\'s frame size with black bars, cropped writes the picture rectangle alone')
    ap.add_argument('--shutter', type=_value_arg(SH.parse_shutter), default=None, metavar='ANGLE',
                    help='synthesize motion blur: every written frame is the average of --shutter-samples finer frames spread over an '
                         'exposure of ANGLE/360 of its frame period, from its own time on (ANGLE in degrees, N or N/D, 0 < ANGLE <= 360; 180 '
                         'is the film look).  Only the time instants those frames need are run, the mix is one launch per batch on the '
                         'GPU and only written frames leave it; samples on the far side of a scene cut (--scene-cut) are left out.  The '
                         'average is taken over the stored (gamma) samples.  S*360/ANGLE must be an integer and F_out/F_in times it at '
                         'most %d.  One rank only; not with --dedup.  Off by default' % R.MAX_RATIO)
    ap.add_argument('--shutter-samples', type=int, default=None, metavar='S',
                    help='with --shutter: the sub-frames averaged per written frame, 1 .. %d (default %d)' % (SH.MAX_SAMPLES, SH.DEFAULT_SAMPLES))
    ap.add_argument('--shutter-window', default=None, choices=list(SH.WINDOWS),
                    help='with --shutter: the weights of the sub-frames: box (default) averages them, triangle weighs sample j of S by '
                         'min(j + 1, S - j) (1,2,2,1 of four), a softer exposure; a group cut short by a scene cut or the end of the '
                         'stream is renormalised by the weights it keeps')
    ap.add_argument('--interlace', type=_value_arg(IL.parse_order), default=None, metavar='tff|bff',
                    help='write interlaced output: frames 2q and 2q+1 of the output stream become the first and the second field of payload '
                         'q (tff: the first is the top field, the even rows; bff: the bottom field), an odd last frame is woven with itself, '
                         'and the header says It / Ib at half the rate, so --fps and --mfi name the FIELD rate: --deinterlace --fps '
                         '60000/1001 --interlace tff turns 50i into 59.94i, --ivtc --fps 60000/1001 --interlace tff film into 59.94i.  '
                         'One launch per batch on the GPU; half the bytes leave it.  With --crop, rows in units of 2 (4 for 4:2:0).  One '
                         'rank only.  Off by default')
    ap.add_argument('--interlace-lowpass', default=None, choices=list(IL.LOWPASS),
                    help='with --interlace: the vertical filter against interline twitter, within each field\'s own frame: linear '
                         '(default, (a + 2c + b + 2) >> 2 over the rows above and below), complex (a five-row filter that keeps more '
                         'detail) or off')
    ap.add_argument('--scale', type=_value_arg(SC.parse_size), default=None, metavar='WxH',
                    help='resize the output on the GPU to W x H: WIDTH FIRST, as ffmpeg\'s -s (--tile is rows first).  Every progressive '
                         'frame the run would write is resampled (behind --shutter\'s mix, in front of --interlace\'s weave, so fields are '
                         'never scaled) by one launch per batch, and the header keeps the display aspect: 720x576 A16:15 becomes 720x480 '
                         'A8:9.  --deinterlace --fps 60000/1001 --scale 720x480 --interlace tff turns 576i50 into 480i59.94.  With --crop '
                         'only under --crop-output cropped; with --interlace H in units of 2 (4 for 4:2:0); a shrink beyond 32 taps an '
                         'axis (16:3 with lanczos3) is refused.  The input\'s own size changes nothing.  Off by default')
    ap.add_argument('--scale-filter', default=None, choices=list(SC.FILTERS),
                    help='with --scale: lanczos3 (default), bicubic (Catmull-Rom) or bilinear; each is stretched for a shrink, so it '
                         'low-passes')
    ap.add_argument('--work-depth', type=int, default=None, choices=list(y4m.DEPTHS), metavar='W',
                    help='the bit depth every stage computes at (8, 10, 12, 14 or 16; at least the input\'s): every payload is promoted to W bits '
                         'on the GPU right behind its upload, so the deinterlacer, the scene scores, the network\'s 16-bit frame path, the shutter\'s '
                         'mix, the scaler and the weave round at W bits and not at the input\'s 8.  Default: the larger of the input\'s depth and '
                         '--out-depth.  The output keeps the INPUT\'s depth unless --out-depth says otherwise: --work-depth 12 alone on an 8-bit '
                         'stream is 8 -> 12 -> 8, dithered.  An 8-bit input needs no --high-depth for it; with --tile it needs '
                         '--tile-high-depth.  fp16 resolves 10 bits fully and about 12 at best: W >= 12 wants --dtype fp32')
    ap.add_argument('--out-depth', type=int, default=None, choices=list(y4m.DEPTHS), metavar='D',
                    help='write the output at D bits (8, 10, 12, 14 or 16; at most the working depth), e.g. --out-depth 10 on an 8-bit stream for a '
                         'Main10 encoder (C420p10).  Below the working depth every written payload is requantised on the GPU as the last '
                         'stage (behind --shutter, --scale and --interlace), so only D-bit payloads leave it; see --dither.  Default: the '
                         'input\'s depth')
    ap.add_argument('--dither', default=None, choices=list(BD.DITHERS),
                    help='with an output depth below the working depth: bayer (default) rounds with an 8x8 ordered-dither threshold, the same '
                         'pattern in every frame and in both fields of an interlaced payload, so a smooth gradient keeps its mean and does not '
                         'band; none rounds half up.  An error where nothing is requantised')
    ap.add_argument('--denoise', nargs='?', type=_value_arg(DN.parse_denoise), const=DN.DEFAULTS, default=None, metavar='A[:B]',
                    help='clean noisy input (DV, 576i / 480i captures, telecined broadcasts) on the GPU in front of the network: every sample '
                         'becomes the rounded mean of itself and of the samples at its position in the frames before and after it, as far '
                         'as they stay close.  Each side walks outward on its own and stops for good at the first sample that differs from '
                         'the frame\'s own by more than A or brings the side\'s summed difference above B (8-bit steps, 0 <= A <= B <= 255, '
                         'one pair for all planes; default %d:%d; A alone means A:2A; 0 changes nothing), so moving edges and cuts are left '
                         'alone.  Behind --ivtc, --crop, --work-depth and --deinterlace (there over fields of the same parity), in front of '
                         'everything else, scene scores included.  Not with --dedup or --deinterlace-mode adaptive.  Off by default'
                         % DN.DEFAULTS)
    ap.add_argument('--deblock', nargs='?', type=_value_arg(DB.parse_deblock), const=DB.DEFAULTS, default=None, metavar='A[:B]',
                    help='smooth the block edges of 8x8-DCT coded input (DV, 576i / 480i captures, DVDs, broadcast captures) on the GPU in front '
                         'of everything else: H.264\'s intra-edge filter on the fixed grid of 8, in every plane.  A line across an edge changes '
                         'only when the step over the edge is below A and the steps next to it are below B (8-bit steps, 0 <= B <= A <= 255, '
                         'one pair for all planes; default %d:%d; A alone means A:(A+3)//4; 0 builds nothing), up to three samples a side '
                         'where the side is flat, so real edges are left alone.  With --deinterlace every field is filtered on its own; '
                         'with --crop the grid stays that of the uncropped stream.  Works with every other switch and any number of ranks.  '
                         'Off by default' % DB.DEFAULTS)
    ap.add_argument('--dering', nargs='?', type=_value_arg(DR.parse_dering), const=DR.DEFAULTS, default=None, metavar='P[:S[:D]]',
                    help='smooth the ringing and mosquito noise beside the edges of 8x8-DCT coded input on the GPU, behind --deblock and in front '
                         'of everything else: AV1\'s constrained directional enhancement filter in every plane.  Every 8x8 block finds its '
                         'dominant direction; samples are smoothed along it with strength P (0 .. %d) and across it with strength S (0 .. %d), and '
                         'a neighbour that differs by more than the strength allows (damping D, %d .. %d) is left out, so real edges stay.  '
                         '8-bit steps, one triple for all planes; default %d:%d:%d (the middle of AV1\'s range, not tuned against this network); '
                         'P alone means P:min((P+1)//2,4):5; 0:0 builds nothing.  With --deinterlace every field is filtered on its own; with '
                         '--crop the grid stays that of the uncropped stream.  Works with every other switch and any number of ranks.  '
                         'Off by default' % ((DR.MAX_P, DR.MAX_S, DR.MIN_D, DR.MAX_D) + DR.DEFAULTS))
    ap.add_argument('--deband', nargs='?', type=_value_arg(BA.parse_deband), const=BA.DEFAULTS, default=None, metavar='T[:R]',
                    help='smooth the bands of coarsely quantised input on the GPU, directly behind --dering and in front of everything else: '
                         'every sample becomes the rounded mean of the samples of its (2R+1)x(2R+1) window that differ from it by less than T, '
                         'in every plane; a step of T or more stays an edge and every even gradient comes back exactly.  T (0 .. %d) in 8-bit '
                         'steps, R (%d .. %d) in samples, one pair for all planes; default %d:%d (not tuned against this network); T alone '
                         'means T:16; 0 builds nothing.  Wants --work-depth 10 or more on 8-bit input: at equal input and working depth a band of '
                         'one code rounds back to itself.  Bands narrower than about R/T stay.  With --deinterlace every field is filtered on its '
                         'own.  Works with every other switch and any number of ranks.  Off by default'
                         % ((BA.MAX_T, BA.MIN_R, BA.MAX_R) + BA.DEFAULTS))
    ap.add_argument('--nlmeans', nargs='?', type=_value_arg(NL.parse_nlmeans), const=NL.DEFAULTS, default=None, metavar='S[:P[:R]]',
                    help='denoise every plane within the frame on the GPU (non-local means in exact integers), behind --dering and in front of '
                         '--deband: every sample becomes the weighted mean of the samples of its (2R+1)x(2R+1) search window, each weighed by '
                         'how little its (2P+1)x(2P+1) patch differs; a hard edge is not seen across.  The answer to noise on anything that moves, '
                         'where --denoise (temporal) stops.  S (0 .. %d) in 8-bit steps, P (%d .. %d) and R (%d .. %d) in samples, one triple for '
                         'all planes; default %d:%d:%d (not tuned against this network); S alone means S:2:5; 0 builds nothing.  A high S costs '
                         'texture; a ramp beside a border or an edge is biased by a few codes.  With --deinterlace every field is filtered on '
                         'its own.  Works with every other switch and any number of ranks.  Off by default'
                         % ((NL.MAX_S, NL.MIN_P, NL.MAX_P, NL.MIN_R, NL.MAX_R) + NL.DEFAULTS))
    ap.add_argument('--denoise-radius', type=int, default=None, metavar='R',
                    help='with --denoise: the frames looked at on each side, 1 .. %d (default %d); costs R frames of lookahead, 2 R fields '
                         'behind --deinterlace' % (DN.MAX_RADIUS, DN.DEFAULT_RADIUS))
    ap.add_argument('--linear-light', nargs='?', const=CL.TRANSFERS[0], default=None, choices=list(CL.TRANSFERS), metavar='TRANSFER',
                    help='mix (--shutter) and resample (--scale) light, not stored samples: the frames behind the network are taken to '
                         'scene-linear light through the inverse of TRANSFER (bt709: the BT.709 / BT.601 / BT.2020-SDR OETF, the default; '
                         'srgb), the mix and the scaler work on 16-bit linear B, G, R planes, and an encode stage takes the result back, so a '
                         'bright object over a dark ground smears as on a real shutter and fine bright detail keeps its brightness when it '
                         'shrinks.  Working depths 8, 10 and 12; without --shutter or --scale it builds nothing.  Off by default')
    ap.add_argument('--out-matrix', default=None, choices=list(CL.OUT_MATRICES),
                    help='YCbCr matrix of the OUTPUT (default: the input\'s, --matrix); auto: BT.709 when the height written is >= 720, else '
                         'BT.601, so --scale 1920x1080 of an SD stream leaves as BT.709.  Y4M has no tag for it')
    ap.add_argument('--out-range', default=None, choices=list(CL.OUT_RANGES),
                    help='range of the OUTPUT (default: the input\'s); the header gets XCOLORRANGE=FULL or LIMITED when the range changes')
    ap.add_argument('--grain', type=_value_arg(_grain_arg(GR.parse_strength)), default=None, metavar='S',
                    help='add synthetic film grain on the GPU to every frame written: --denoise, the network, --shutter and --scale leave a '
                         'picture cleaner than any camera original, which looks synthetic next to untouched material and bands at 8 and 10 '
                         'bits.  S is the grain\'s standard deviation in 8-bit code values at the curve\'s peak, 0 .. 8, a decimal in sixteenths '
                         '(1 to 2 is fine film, 4 is coarse; 0 builds nothing).  Behind --shutter, --scale and --linear-light\'s encode, which would '
                         'average it away, in front of --interlace (both fields get their own grain) and --out-depth\'s dither; one launch per '
                         'batch.  Grain never leaves the legal range.  Every frame gets fresh grain from (seed, frame number), so the bytes '
                         'do not depend on --batch.  One rank only.  Off by default')
    ap.add_argument('--grain-size', type=int, default=None, choices=[0, 1, 2], metavar='R',
                    help='with --grain: how coarse the grain is: 0 white noise, 1 (default) a 3x3, 2 a 5x5 binomial blur of it; the '
                         'strength stays S')
    ap.add_argument('--grain-chroma', type=_value_arg(_grain_arg(GR.parse_chroma)), default=None, metavar='C',
                    help='with --grain: the strength of the chroma planes\' grain relative to luma, 0 .. 1 in sixteenths (default 0.5; 0: '
                         'luma only)')
    ap.add_argument('--grain-curve', default=None, choices=list(GR.CURVES),
                    help='with --grain: film (default) follows the frame\'s own luma, full strength in the midtones and a quarter at black '
                         'and white; flat is the same everywhere')
    ap.add_argument('--grain-seed', type=_value_arg(GR.parse_seed), default=None, metavar='N',
                    help='with --grain: a 32-bit seed (default 0); the same seed gives the same bytes')
    ap.add_argument('--lut', default=None, metavar='FILE.cube',
                    help='apply a 3D colour LUT (Adobe / Resolve .cube, LUT_3D_SIZE 2 .. 65, domain 0 .. 1) on the GPU to every frame written: '
                         'HDR10 or HLG to SDR, BT.2020 to BT.709, camera log to display, a legaliser or a look, all as data.  Tetrahedral '
                         'interpolation in exact integers over R\'G\'B\' at full chroma resolution and the working depth (8, 10 or 12 bits, see '
                         '--work-depth), behind --shutter and --scale and in front of the encode (--out-matrix, --out-range), --grain, '
                         '--interlace and --out-depth; one launch per batch.  The bars of --crop-output pad stay exact black.  Off by default')
    T.add_arguments(ap)
    return ap


def main(argv=None):
    """``python -m demfi_amd.video IN OUT`` -- x M interpolation of a Y4M stream, or retiming to ``--fps``; ``-`` is stdin / stdout.
    The first and the last input frame have no output (as in the reference's test_custom): n frames in, (n-3)*M + 1 out, at M
    times the frame rate; with --fps, floor((n-3)*F_out/F_in) + 1 out at F_out.  --full-length: n*M (ceil(n*F_out/F_in)) out,
    output frame 0 at input frame 0."""
    import json
    import time
    a = parser().parse_args(argv)
    if a.fps is None and a.mfi is None:
        a.mfi = 8
    try:
        check_deinterlace_mode(a.deinterlace, a.deinterlace_mode, a.dedup or None)
        check_ivtc(a.ivtc, a.deinterlace)
        TC.check_params(a.ivtc_cthresh, a.ivtc_combpel, a.ivtc_combed)
        crop_kw = {k: v for k, v in (('crop', a.crop), ('crop_limit', a.crop_limit), ('crop_noise', a.crop_noise),
                                     ('crop_probe', a.crop_probe), ('crop_output', a.crop_output)) if v is not None}
        check_crop(*(crop_kw.get(k, d) for k, d in (('crop', None), ('crop_limit', LB.DEFAULT_LIMIT), ('crop_noise', LB.DEFAULT_NOISE),
                                                    ('crop_probe', LB.DEFAULT_PROBE), ('crop_output', 'pad'))))
        if a.crop == 'auto' and not (_is_regular(a.input) and os.path.isfile(a.input) and _is_regular(a.output)):
            raise ValueError(AUTO_NEEDS_A_FILE + ' (and a regular output file)')
        check_shutter_window(check_shutter(a.shutter, a.shutter_samples, a.dedup or None), a.shutter_window)
        check_interlace(a.interlace, a.interlace_lowpass)
        check_scale(a.scale, a.scale_filter, a.crop, crop_kw.get('crop_output', 'pad'))
        check_depths(a.work_depth, a.out_depth, a.dither)
        check_denoise(a.denoise, a.denoise_radius, a.dedup or None, a.deinterlace_mode)
        check_deblock(a.deblock)
        check_dering(a.dering)
        check_deband(a.deband)
        check_nlmeans(a.nlmeans)
        check_colour(a.linear_light, a.out_matrix, a.out_range, auto=True)
        grain = check_grain(a.grain, a.grain_size, a.grain_chroma, a.grain_curve, a.grain_seed)
        lut = check_lut(a.lut, check_depths(a.work_depth, a.out_depth, a.dither)[0])
    except ValueError as e:
        parser().error(str(e))
    shutter_kw = {k: v for k, v in (('shutter', a.shutter), ('shutter_samples', a.shutter_samples), ('interlace', a.interlace),
                                    ('interlace_lowpass', a.interlace_lowpass), ('scale', a.scale),
                                    ('scale_filter', a.scale_filter), ('work_depth', a.work_depth), ('out_depth', a.out_depth),
                                    ('dither', a.dither), ('shutter_window', a.shutter_window), ('denoise', a.denoise),
                                    ('denoise_radius', a.denoise_radius), ('linear_light', a.linear_light), ('out_matrix', a.out_matrix),
                                    ('out_range', a.out_range), ('grain', a.grain), ('grain_size', a.grain_size),
                                    ('grain_chroma', a.grain_chroma), ('grain_curve', a.grain_curve), ('grain_seed', a.grain_seed),
                                    ('deblock', a.deblock), ('dering', a.dering), ('deband', a.deband), ('lut', lut),
                                    ('nlmeans', a.nlmeans))
                  if v is not None}
    rank, local, world = (int(os.environ.get(k, d)) for k, d in (('RANK', 0), ('LOCAL_RANK', 0), ('WORLD_SIZE', 1)))
    try:
        check_one_rank(world, dedup=a.dedup, ivtc=a.ivtc, shutter=a.shutter, interlace=a.interlace, grain=grain)
    except ValueError as e:
        raise SystemExit('demfi_amd.video: ' + str(e))
    if world > 1 and not (_is_regular(a.input) and os.path.isfile(a.input) and _is_regular(a.output)):
        raise SystemExit('demfi_amd.video: with %d ranks IN and OUT must be regular files (ranks write at byte offsets)' % world)
    out_fd = None
    if a.output == '-':
        # the stream owns stdout: anything a library prints goes to stderr instead
        out_fd = os.dup(1)
        os.dup2(2, 1)
        sys.stdout = sys.stderr
    if not torch.cuda.is_available():
        raise SystemExit('demfi_amd.video: no GPU visible -- the forward path is HIP-only (no CPU fallback)')
    from . import DeMFInet, HyperParams, synthetic_state_dict
    from .weights import load_checkpoint
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    D.init(world, rank, local)
    model = DeMFInet(HyperParams(gpu=local), dtype=torch.float16 if a.dtype == 'fp16' else torch.float32)
    if rank == 0:
        model.load_state_dict(load_checkpoint(a.checkpoint) if a.checkpoint else synthetic_state_dict(0))
    model = model.to(dev).eval()
    D.broadcast_state_dict(model, world, device=dev)
    vr = VideoRunner(model, a.n_tst, a.mfi, batch=a.batch, matrix=a.matrix, fps=a.fps, scene_cut=a.scene_cut, full_length=a.full_length,
                     tile=a.tile, tile_margin=a.tile_margin, high_depth=a.high_depth, layouts=a.any_layout, dedup=a.dedup or None,
                     dedup_max_hold=a.dedup_max_hold, tile_high_depth=a.tile_high_depth, deinterlace=a.deinterlace,
                     deinterlace_mode=a.deinterlace_mode, ivtc=a.ivtc, ivtc_cthresh=a.ivtc_cthresh, ivtc_combpel=a.ivtc_combpel,
                     ivtc_combed=a.ivtc_combed, down=a.downconvert, **crop_kw, **shutter_kw)
    t0 = time.perf_counter()
    if world > 1 or a.crop == 'auto':                        # the pre-pass seeks: regular files
        nw, nf = vr.run_file(a.input, a.output, world, rank)
    else:
        src = sys.stdin.buffer if a.input == '-' else open(a.input, 'rb')
        dst = os.fdopen(out_fd, 'wb') if out_fd is not None else open(a.output, 'wb')
        try:
            nw, nf = vr.run_stream(src, dst)
        finally:
            dst.close()
            if src is not sys.stdin.buffer:
                src.close()
    torch.cuda.synchronize()
    dt = D.max_over_ranks(time.perf_counter() - t0, dev)
    counts = [float(nw), float(nf), float(vr.last_st_frames), float(vr.last_instants[0]), float(vr.last_instants[1]),
              float(vr.last_cut_windows), float(vr.last_depth_promoted), float(vr.last_depth_requantised), float(vr.last_denoised), float(vr.last_deblocked),
              float(vr.last_deringed), float(vr.last_debanded), float(vr.last_nlm_filtered)]
    tw, tf, tst, ti, tp, tc, tdp, tdq, tdn, tdb, tdr, tba, tnl = (D.sum_over_ranks(counts, dev).tolist() if world > 1 else counts)
    if rank == 0:
        if a.crop is not None:
            print('demfi_amd.video: ' + vr.crop_report(), file=sys.stderr)
        if tw == 0:
            print('demfi_amd.video: %s: no window, only the header was written' %
                  ('no input frame' if a.full_length else 'fewer than 4 input frames'), file=sys.stderr)
        extra = {'shutter': {'angle': str(a.shutter), 'samples': vr.last_shutter[0], 'fine_per_written': vr.last_shutter[1]}} if a.shutter else {}
        if a.shutter_window is not None:
            extra['shutter']['window'] = vr.last_shutter_window
        if a.downconvert:
            extra['windows_skipped'] = vr.last_windows_skipped
        if a.interlace is not None:
            extra['interlace'] = {'order': vr.last_interlace, 'lowpass': vr.interlace[1], 'carried': vr.last_interlace_carried}
        if a.denoise is not None:
            extra['denoise'] = {'a': vr.denoise[0], 'b': vr.denoise[1], 'radius': vr.denoise[2], 'frames': int(tdn)}
        if a.deblock is not None:
            extra['deblock'] = {'a': a.deblock[0], 'b': a.deblock[1], 'payloads': int(tdb)}
        if a.dering is not None:
            extra['dering'] = {'p': a.dering[0], 's': a.dering[1], 'd': a.dering[2], 'payloads': int(tdr)}
        if a.deband is not None:
            extra['deband'] = {'t': a.deband[0], 'r': a.deband[1], 'payloads': int(tba)}
        if a.nlmeans is not None:
            extra['nlmeans'] = {'s': a.nlmeans[0], 'p': a.nlmeans[1], 'r': a.nlmeans[2], 'payloads': int(tnl)}
        if a.scale is not None:
            extra['scale'] = {'size': '%dx%d' % vr.scale[:2], 'filter': vr.scale[2], 'resized': vr.last_scale is not None,
                              'payloads': vr.last_scale_payloads}
        if a.grain is not None:
            g = vr.last_grain
            extra['grain'] = {'payloads': vr.last_grain_payloads} if g is None else {
                'strength': g[0] / 16, 'size': g[1], 'chroma': g[2] / 16, 'curve': g[3], 'seed': g[4], 'payloads': vr.last_grain_payloads}
        if a.lut is not None:
            extra['lut'] = {'size': vr.lut.n, 'payloads': vr.last_lut_payloads}
        if vr.last_colour is not None:
            extra['colour'] = {'linear_light': vr.last_colour[0], 'matrix': vr.last_colour[1], 'range': 'full' if vr.last_colour[2] else 'limited',
                               'encoded': vr.last_colour_encoded}
        depth = vr.last_depth                        # the depth written; with a depth switch the whole story
        if any(v is not None for v in (a.work_depth, a.out_depth, a.dither)) and vr.last_depths is not None:
            depth = {'in': vr.last_depths[0], 'work': vr.last_depths[1], 'out': vr.last_depths[2], 'dither': vr.last_depths[3],
                     'promoted': int(tdp), 'requantised': int(tdq)}
        print(json.dumps({**extra, 'windows': int(tw), 'frames_written': int(tf), 'seconds': round(dt, 2), 'ranks': world,
                          'St_frames_per_s': round(tst / dt, 2) if dt > 0 else None,
                          'frames_per_s': round(tf / dt, 2) if dt > 0 else None,
                          'fps_out': str(vr.last_fps_out) if vr.last_fps_out is not None else None,
                          'instants_run': int(ti), 'instants_padded': int(tp), 'cut_windows': int(tc), 'dups': len(vr.last_dups),
                          'tiles': vr.last_plan.n_tiles if vr.last_plan is not None else 1,
                          'tile': vr.last_plan.label() if vr.last_plan is not None else None, 'depth': depth, 'layout': vr.last_layout,
                          'fields': vr.last_fields, 'ivtc_matches': vr.last_matches if a.ivtc else None,
                          'ivtc_dropped': vr.last_dropped if a.ivtc else None, 'ivtc_combed': vr.last_combed if a.ivtc else None,
                          'crop': list(vr.last_crop) if vr.last_crop is not None else None,
                          'crop_probe_seconds': round(vr.last_crop_seconds, 3) if a.crop == 'auto' else None,
                          'weights': os.path.basename(a.checkpoint) if a.checkpoint else 'synthetic_state_dict(0) (random init: no checkpoint given)',
                          'out': a.output}), file=sys.stderr)
    D.finalize()


if __name__ == '__main__':
    main()
