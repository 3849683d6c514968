"""Switch an importable transflow installation over to this backend without editing it.

    import transflow_amd.dropin as dropin
    dropin.install()          # before transflow.pipeline builds its sources
    ...                       # transflow runs as usual; pipeline.py is unchanged
    dropin.uninstall()

`install()` replaces the two factories pipeline.py calls
(transflow/pipeline.py:325 FlowSource.from_args, :445 Compositor.from_args) with
dispatchers that build HipFlowSource / HipCompositor when the request is one this
backend serves -- a video path (or webcam index) with the Farnebäck method, or Horn-Schunck when
`install(horn_schunck=True)` asks for it, or Lucas-Kanade when `install(lucas_kanade=True)` does, or LiteFlowNet when
`install(liteflownet=<weights>)` gives the network's weights (flow mask and the
scale/threshold/clip filters, the convolution kernel and per-pixel polar expressions included), or codec motion
vectors (`use_mvs`, transflow's `-m`) when `install(motion_vectors=True)` asks for them, layers of
any of the reference's classes (`moveref`, `sum`, `static`, `introduction`) -- and fall through to
the reference's own factory otherwise (other flow methods, polar expressions that are
not per-pixel formulas).
`.flow.zip` archives are served too (their flows are post-processed on the GPU).
`install(pixmaps=True)` replaces a third factory, PixmapSource.from_args (pipeline.py:382): still pixmap sources are then
transflow_amd/pixmap.py's; video pixmap sources stay the reference's.
INTEGRATION.md shows the three-line patch a maintainer would add instead.
"""
from __future__ import annotations

import os
import re

_saved = {}
_pixmap_options = {"stills": False, "mjpeg": False, "png": False, "mjpeg_parallel": False, "yuv": False, "yuv_matrix": "bt601"}   # what the installed pixmap factory serves
_saved_export = []      # (the reference's pipeline module, its NumpyOutput, deviceflow.DEVICE_ROUND) while device_flow_export is on
_saved_seam = []        # (the pipeline module, its upscale_array, render1d, render2d, the merging dict's entries,
                        # deviceflow.DEVICE_VIEW, the FlowView) while device_seam is on


def _served_config(cv_config, horn_schunck: bool, lucas_kanade: bool = False, liteflownet=None) -> bool:
    """Whether the flow method a cv_config (a JSON path, a CvFlowConfig object, None) names is one this backend runs."""
    from .config import HornSchunckConfig, flow_config_from_arg
    try:                        # config.METHODS says which methods are served, and behind which of these opt-ins
        cfg = flow_config_from_arg(cv_config, lucas_kanade=lucas_kanade, liteflownet=liteflownet)
    except ValueError:          # another flow method: the reference's own source
        return False
    # (the library serves Horn-Schunck either way; the drop-in routes it here only on request)
    return horn_schunck or not isinstance(cfg, HornSchunckConfig)


def _is_mjpeg(path) -> bool:
    from .jpegdec import MJPEG_EXTS
    return isinstance(path, str) and os.path.splitext(path)[1].lower() in MJPEG_EXTS and os.path.isfile(path)


def _is_png_sequence(path) -> bool:
    from .pngdec import is_png_sequence
    return is_png_sequence(path)


def _is_y4m(path) -> bool:
    from .yuvdec import is_y4m
    return is_y4m(path)


def _flow_from_args(original, horn_schunck=False, lucas_kanade=False, liteflownet=None, motion_vectors=False,
                    device_flow_replay=False, mjpeg_inputs=False, png_inputs=False, mjpeg_parallel=False, yuv_inputs=False,
                    yuv_input_matrix="bt601", resident_steps=False):
    from .flow import HipFlowSource

    def from_args(cls, flow_path, use_mvs=False, mask_path=None, kernel_path=None, cv_config=None,
                  flow_filters=None, size=None, direction=None, seek_ckpt=None, seek_time=None,
                  duration_time=None, repeat=1, lock_expr=None, lock_mode="stay"):
        # (a motion-vector source reads no cv_config: source.py:400-402)
        served = isinstance(flow_path, str) and (motion_vectors if use_mvs else cv_config != "window")
        if served and flow_filters is not None and "polar" in flow_filters:
            try:                                   # polar expressions the device cannot run stay the reference's
                from .flow import FlowFilter
                for part in flow_filters.strip().split(";"):
                    FlowFilter.from_string(part)
            except NotImplementedError:
                served = False
        if served and not use_mvs and not _served_config(cv_config, horn_schunck, lucas_kanade, liteflownet):
            served = False
        if not served:
            return original(flow_path, use_mvs=use_mvs, mask_path=mask_path, kernel_path=kernel_path,
                            cv_config=cv_config, flow_filters=flow_filters, size=size, direction=direction,
                            seek_ckpt=seek_ckpt, seek_time=seek_time, duration_time=duration_time, repeat=repeat,
                            lock_expr=lock_expr, lock_mode=lock_mode)
        if mjpeg_inputs and not use_mvs and _is_mjpeg(flow_path):   # a raw MJPEG stream: its frames are decoded on the device
            from .jpegdec import MjpegFrameProvider
            flow_path = MjpegFrameProvider(flow_path, size=size, parallel_scan=mjpeg_parallel)
        elif png_inputs and not use_mvs and _is_png_sequence(flow_path):   # a PNG frame sequence: likewise
            from .pngdec import PngSequenceFrameProvider
            flow_path = PngSequenceFrameProvider(flow_path, size=size)
        elif yuv_inputs and not use_mvs and _is_y4m(flow_path):   # a Y4M file: its planes go up, the device converts them
            from .yuvdec import Y4mFrameProvider
            flow_path = Y4mFrameProvider(flow_path, size=size, matrix=yuv_input_matrix,
                                         chroma="linear" if yuv_inputs == "linear" else "replicate")
        return HipFlowSource.from_args(flow_path, use_mvs, mask_path, kernel_path, cv_config, flow_filters, size,
                                       direction, seek_ckpt, seek_time, duration_time, repeat, lock_expr, lock_mode,
                                       lucas_kanade=lucas_kanade, liteflownet=liteflownet,
                                       archive_device_inflate=device_flow_replay, resident_steps=resident_steps)

    return classmethod(from_args)


def _compositor_from_args(original, lazy_frames=False, jpeg_frames=None, png_frames=False, png_code="fixed",
                          jpeg_optimize=False, jpeg_subsampling=None, yuv_frames=None, yuv_matrix=None, yuv_range=None,
                          reset_rng="numpy"):
    from .compositor import LAYER_CLASSES, HipCompositor

    def from_args(cls, height, width, layer_configs, background_color="#ffffff"):
        if all(getattr(c, "classname", None) in LAYER_CLASSES for c in layer_configs):
            return HipCompositor.from_args(height, width, layer_configs, background_color=background_color, rng=reset_rng,
                                           lazy_frames=lazy_frames, jpeg_frames=jpeg_frames, png_frames=png_frames,
                                           png_code=png_code, jpeg_optimize=jpeg_optimize,
                                           jpeg_subsampling=jpeg_subsampling, yuv_frames=yuv_frames, yuv_matrix=yuv_matrix,
                                           yuv_range=yuv_range)
        return original(height, width, layer_configs, background_color=background_color)

    return classmethod(from_args)


def _output_from_args(original, quality, optimize=False, subsampling=2):
    from .output import (HipFramesOutput, HipMjpegFileOutput, HipMjpegOutput, RawFramesOnly, jpeg_template, mjpeg_address,
                         mjpeg_file_path)

    def from_args(cls, path, width, height, framerate=None, vcodec="h264", execute=False, replace=False, initial_counter=0):
        address = mjpeg_address(path)
        if address is not None:
            return HipMjpegOutput(address[0], address[1], width, height, 30 if framerate is None else framerate, quality,
                                  optimize=optimize, subsampling=subsampling)
        if jpeg_template(path):     # `out/%05d.jpg`: a file a frame
            return HipFramesOutput(path, width, height, initial_counter, execute, quality=quality, subsampling=subsampling,
                                   optimize=optimize)
        if mjpeg_file_path(path):   # `out.mjpeg`: the files back to back, what the device decoder's inputs are read as
            return HipMjpegFileOutput(path, width, height, 30 if framerate is None else framerate, quality,
                                      subsampling=subsampling, optimize=optimize, execute=execute, replace=replace)
        # the reference's own output; it takes pixels, and says so if it is given a file
        return RawFramesOnly(original(path, width, height, framerate=framerate, vcodec=vcodec, execute=execute,
                                      replace=replace, initial_counter=initial_counter))

    return classmethod(from_args)


def _png_output_from_args(original):
    from .output import HipFramesOutput, RawFramesOnly, png_template

    def from_args(cls, path, width, height, framerate=None, vcodec="h264", execute=False, replace=False, initial_counter=0):
        if not png_template(path):  # the reference's own output; it takes pixels, and says so if it is given a file
            return RawFramesOnly(original(path, width, height, framerate=framerate, vcodec=vcodec, execute=execute,
                                          replace=replace, initial_counter=initial_counter))
        return HipFramesOutput(path, width, height, initial_counter, execute)

    return classmethod(from_args)


def _yuv_output_from_args(original, layout, matrix, range):
    from .output import HipFfmpegOutput, HipY4mOutput, RawFramesOnly, ffmpeg_path, y4m_path

    def from_args(cls, path, width, height, framerate=None, vcodec="h264", execute=False, replace=False, initial_counter=0):
        if y4m_path(path):          # `out.y4m`: the planes in the uncompressed container
            return HipY4mOutput(path, width, height, 30 if framerate is None else framerate, layout, matrix, range,
                                execute=execute, replace=replace)
        if ffmpeg_path(path):       # what video_output.py:59-60 gives to FFmpegVideoOutput
            return HipFfmpegOutput(path, width, height, 30 if framerate is None else framerate, vcodec, execute, replace,
                                   layout=layout, matrix=matrix, range=range)
        # the reference's own output; it takes pixels, and says so if it is given planes
        return RawFramesOnly(original(path, width, height, framerate=framerate, vcodec=vcodec, execute=execute,
                                      replace=replace, initial_counter=initial_counter))

    return classmethod(from_args)


def _pixmap_from_args(original, stills=True, mjpeg_inputs=False, png_inputs=False, mjpeg_parallel=False, yuv_inputs=False,
                      yuv_input_matrix="bt601"):
    from .pixmap import HipPixmapSource

    def from_args(cls, path, size, seek=None, seed=None, seek_time=None, alteration_path=None, repeat=1, flow_path=None):
        still = stills and re.match(HipPixmapSource.STILL_RE, path.lower().strip()) is not None
        image = stills and os.path.isfile(path) and os.path.splitext(path)[1].lower() in HipPixmapSource.IMAGE_EXTS
        video = (mjpeg_inputs and _is_mjpeg(path)) or (png_inputs and _is_png_sequence(path)) or (yuv_inputs and _is_y4m(path))
        if not (still or image or video):                                  # a video: the reference's CvPixmapSource
            return original(path, size, seek=seek, seed=seed, seek_time=seek_time, alteration_path=alteration_path,
                            repeat=repeat, flow_path=flow_path)
        return HipPixmapSource.from_args(path, size, seek, seed, seek_time, alteration_path, repeat, flow_path,
                                         mjpeg_parallel_scan=mjpeg_parallel, y4m_inputs=yuv_inputs, y4m_matrix=yuv_input_matrix)

    return classmethod(from_args)


def _seam_wrappers(originals, view):
    """The four names device_seam replaces: each takes the device route for float32 DeviceFlows whose device copy is
    current (transflow_amd/seam.py) and calls the original otherwise."""
    from . import seam
    upscale_original, render1d_original, render2d_original, merging = originals

    def upscale_array(arr, wf, hf):
        return seam.upscale(arr, wf, hf, fallback=upscale_original)

    def render1d(arr, scale=1, colors=None, binary=False):
        if isinstance(arr, seam.FlowMagnitude) and arr.resident:
            return view.view_magnitude(arr, scale, colors, binary)
        return render1d_original(arr, scale, colors, binary)

    def render2d(arr, scale=1, colors=None):
        if seam.is_resident(arr):
            return view.view2d(arr, scale, colors)
        return render2d_original(arr, scale, colors)

    def merger(kind, original):
        return lambda flows: seam.merge(kind, flows, fallback=original)

    return upscale_array, render1d, render2d, {k: merger(k, f) for k, f in merging.items() if k in seam.MERGE_KINDS}


def install(flow: bool = True, compositor: bool = True, lazy_frames: bool = False, horn_schunck: bool = False,
            lucas_kanade: bool = False, liteflownet=None, motion_vectors: bool = False, pixmaps: bool = False,
            jpeg_frames: int | None = None, png_frames: bool = False, device_flow_export=False,
            device_flow_replay: bool = False, mjpeg_inputs=False, png_inputs: bool = False, png_code: str = "fixed",
            jpeg_optimize: bool = False, jpeg_subsampling=None, yuv_frames: str | None = None, yuv_matrix: str | None = None,
            yuv_range: str | None = None, yuv_inputs=False, yuv_input_matrix: str = "bt601",
            resident_steps: bool = False, device_seam: bool = False, reset_rng: str = "numpy") -> None:
    """Needs `transflow` importable.  Idempotent.  horn_schunck: flow sources of the Horn-Schunck method are this
    backend's too (transflow_amd/hornschunck.py; by default they stay the reference's).  lucas_kanade: likewise for
    the Lucas-Kanade method ("lukas-kanade", transflow_amd/lucaskanade.py).  liteflownet: the network's weights (a path
    to the state dict, or a dict of arrays): flow sources of the "liteflownet" method are then this backend's
    (transflow_amd/liteflownet.py); without them they stay the reference's.  For these three methods the keys
    "hip_resident" (flows and the previous output stay on the device through the post-process), "hip_device_flows" and
    "hip_batch" travel in the cv_config JSON, as Farnebäck's keys do (transflow_amd/config.py): no argument here.
    motion_vectors: `use_mvs` requests (codec
    motion vectors, transflow's -m) are this backend's too (transflow_amd/motionvectors.py; PyAV still decodes); by
    default they stay the reference's.  lazy_frames: the compositors built for the pipeline return
    DeviceFrames from render() (transflow_amd/deviceframe.py): the pipeline's `oq.put(frame)` (pipeline.py:518-522) then
    pickles the frame -- and waits for its download -- in the queue's feeder thread, beside the next update.
    pixmaps: still pixmap sources (colours, the noises, gradient, images, a video's first frame) are this backend's
    (transflow_amd/pixmap.py): made once, kept on the device, taken by the layers of a compositor of the same process by
    address; across a process boundary they travel as host arrays.  By default they stay the reference's.
    jpeg_frames: a JPEG quality -- the compositors built for the pipeline return JpegFrames from render()
    (transflow_amd/jpeg.py: encoded on the device, only the file comes down and crosses to the output process), and
    VideoOutput.from_args (pipeline.py's output process) builds a HipMjpegOutput (transflow_amd/output.py) for `mjpeg...`
    paths, a HipFramesOutput for `%d` templates that end in .jpg / .jpeg (a file a frame) and a HipMjpegFileOutput for
    paths with a .mjpeg / .mjpg extension (a raw MJPEG stream, the form `mjpeg_inputs` reads); any other output is the
    reference's own and raises a TypeError that names this option when it is fed a JpegFrame.  Not together with lazy_frames.  By default (None) nothing of this is touched.
    jpeg_optimize: with jpeg_frames, the files carry the frame's own Huffman tables (JpegEncoder(optimize=True),
    DESIGN.md section 15; libjpeg's optimize_coding): smaller files of the same pixels, and a raw frame that reaches the
    MJPEG output is encoded on the host with the same setting; False (the default) keeps writing the bytes it wrote before.
    jpeg_subsampling: with jpeg_frames, the files' chroma layout -- 0 / "4:4:4", 1 / "4:2:2" or 2 / "4:2:0"
    (JpegEncoder(subsampling=...)): 4:4:4 keeps the one-pixel colour edges of a rendered frame that
    4:2:0 averages; a raw frame that reaches one of the three JPEG outputs is encoded on the host with the same layout;
    None (the default) keeps writing 4:2:0, the bytes it wrote before.
    png_frames: the compositors built for the pipeline return PngFrames from render() (transflow_amd/png.py: the
    lossless file, made on the device), and VideoOutput.from_args builds a HipFramesOutput (transflow_amd/output.py) for
    `%d` templates that end in `.png`; any other output is the reference's own and raises a TypeError that names this
    option when it is fed a PngFrame.  Not together with jpeg_frames or lazy_frames.  By default nothing of this is
    touched.  png_frames="indexed": the same, and the files carry the band index (PngEncoder(index=True), DESIGN.md
    section 20) that lets `png_inputs` decode them on the device; plain True keeps writing the bytes it wrote before.
    png_code="frame": with png_frames (True or "indexed"), the files are coded with the frame's own literal/length code
    and a band that would not shrink is stored (PngEncoder(code="frame")): smaller files of the
    same pixels, which any decoder and `png_inputs` read; "fixed" (the default) keeps writing the bytes it wrote before.
    device_flow_export: the flow export (`--export-flow`, `--export-rounded-flow`) writes its `.flow.zip` through
    archive.DeviceFlowArchiveWriter, put where pipeline.py:369 finds NumpyOutput: a DeviceFlow is deflated on the device
    (transflow_amd/flowzip.py) and only the member comes down; and `numpy.round(flow).astype(int)` (pipeline.py:506) of a
    DeviceFlow is computed on the device too (deviceflow.DEVICE_ROUND).  Host arrays are written as before.
    device_flow_export="indexed": the same, and the writer leaves a band index in the archive
    (DeviceFlowArchiveWriter(index=True)); plain True keeps writing the bytes it wrote before.
    device_flow_replay: the archive source FlowSource.from_args builds for a `.flow.zip` path is
    archive.ArchiveFlowSource(device_inflate=True): members with a band index are inflated on the device
    (transflow_amd/flowunzip.py) straight into the flow that is post-processed there; members without one, and every
    member while a lock expression or (without resident_steps) a polar filter or a kernel needs the raw flow on the
    host, are read as before.
    mjpeg_inputs: an existing file with extension .mjpeg / .mjpg (a raw MJPEG stream) is decoded on the device
    (transflow_amd/jpegdec.py), as a flow source's video (a MjpegFrameProvider under the HipFlowSource) and as a pixmap
    source (HipMjpegPixmapSource); by default such paths stay the reference's, like every other video.
    mjpeg_inputs="parallel": the same, and frames without a restart interval -- what ffmpeg, OpenCV and cameras write --
    are decoded on the device too (MjpegFrameProvider(parallel_scan=True)) instead of by Pillow; plain True keeps
    routing them as before.
    png_inputs: a path with a `%...d` field that ends in .png and whose first frame (0 or 1) exists -- a PNG frame
    sequence -- is read by transflow_amd/pngdec.py, as a flow source's video (a PngSequenceFrameProvider under the
    HipFlowSource) and as a pixmap source (HipPngSequencePixmapSource): frames with a band index are decoded on the
    device, the others by Pillow; by default such paths stay the reference's.
    yuv_frames: a layout, "yuv444p", "yuv422p", "yuv420p" or "nv12" -- the compositors built for the pipeline return
    YuvFrames from render() (transflow_amd/yuv.py: the planes a video encoder takes, converted on the device; half the
    RGB frame's bytes come down at 4:2:0), and VideoOutput.from_args builds a HipFfmpegOutput (transflow_amd/output.py)
    for every path the reference gives to FFmpegVideoOutput (video_output.py:59-60) and a HipY4mOutput for paths that end
    in .y4m; any other output is the reference's own and raises a TypeError that names this option when it is fed a
    YuvFrame.  yuv_matrix ("bt601", the default, or "bt709") and yuv_range ("tv", the default, or "pc") only with
    yuv_frames.  Not together with jpeg_frames, png_frames or lazy_frames.  By default (None) nothing of this is touched.
    yuv_inputs: an existing file whose name ends in .y4m (YUV4MPEG2: what `ffmpeg -i any.mp4 out.y4m` and HipY4mOutput
    write) is read by transflow_amd/yuvdec.py, as a flow source's video (a Y4mFrameProvider under the HipFlowSource; not
    with use_mvs) and as a pixmap source (HipY4mPixmapSource): the planes go up the link as they are and the device
    converts them to pixels (these are not swscale's pixels).  True expands the chroma by
    replication, "linear" by the centre-sited triangle filter; any other value is a ValueError.  yuv_input_matrix
    ("bt601", the default, or "bt709") is the matrix the file was made with: Y4M has no tag for it.  By default such
    paths stay the reference's, like every other video.
    resident_steps: the flow sources built for the pipeline are made with `resident_steps=True` (FlowSource.__init__,
    DESIGN.md section 10): a convolution kernel (`--kernel`) and `polar` flow filters then stay on the device wherever the
    source has a resident tail -- Farnebäck, a method with "hip_resident", motion vectors, device_flow_replay -- and a
    source with a float64 kernel and "hip_device_flows" yields float64 DeviceFlows.  By default such sources take the host
    route, as before.
    device_seam: the steps of the main loop between the flow sources and the compositor keep a DeviceFlow on the device
    (transflow_amd/seam.py): the pipeline module's `upscale_array`, `render1d` and `render2d` and the
    entries of `Pipeline.FLOW_MERGING_FUNCTIONS` are replaced by wrappers that serve float32 DeviceFlows whose device copy
    is current -- merged and upscaled flows are DeviceFlows again, `--view-flow` and `--view-flow-magnitude` frames are
    rendered from the flow where it is (deviceflow.DEVICE_VIEW) and leave in the form this call's frame options
    (lazy_frames, jpeg_frames, png_frames, yuv_frames and theirs) give the compositor's frames -- and call the
    reference's function for everything else.  By default nothing of this is touched.
    reset_rng: where the compositors built for the pipeline draw a random reset's field (`reset_mode: "random"`,
    reference.py:59) -- HipCompositor.from_args' `rng`.  "numpy" (the default): numpy.random.random on the host, as
    before.  "mt19937": numpy's own global stream drawn on the device (transflow_amd/mtstream.py):
    the same frames for the same numpy seed, no draw on the host, no upload, and a lone moveref layer fed DeviceFlows
    takes the one-launch step.  "device": the library's counter-based generator -- other frames."""
    from .compositor import RNGS
    if reset_rng not in RNGS:
        raise ValueError(f"reset_rng is one of {', '.join(RNGS)}, not {reset_rng!r}")
    if not isinstance(yuv_inputs, bool) and not (isinstance(yuv_inputs, str) and yuv_inputs == "linear"):
        raise ValueError(f"yuv_inputs is True or \"linear\", not {yuv_inputs!r}")
    if yuv_input_matrix not in ("bt601", "bt709"):
        raise ValueError(f"yuv_input_matrix is \"bt601\" or \"bt709\", not {yuv_input_matrix!r}")
    if yuv_frames is None:
        if yuv_matrix is not None or yuv_range is not None:
            raise ValueError("yuv_matrix and yuv_range are for yuv_frames: without them no YUV frame is made")
    else:
        if jpeg_frames is not None or png_frames or lazy_frames:
            raise ValueError("yuv_frames excludes jpeg_frames, png_frames and lazy_frames")
        from .yuv import check_options
        yuv_matrix = "bt601" if yuv_matrix is None else yuv_matrix
        yuv_range = "tv" if yuv_range is None else yuv_range
        check_options(yuv_frames, yuv_matrix, yuv_range)
    if jpeg_frames is not None and lazy_frames:
        raise ValueError("jpeg_frames and lazy_frames exclude each other")
    if png_frames and (jpeg_frames is not None or lazy_frames):
        raise ValueError("png_frames excludes jpeg_frames and lazy_frames")
    if png_code not in ("fixed", "frame"):
        raise ValueError(f"png_code is \"fixed\" or \"frame\", not {png_code!r}")
    if png_code != "fixed" and not png_frames:
        raise ValueError("png_code is for png_frames: without them no PNG is written")
    if jpeg_optimize and jpeg_frames is None:
        raise ValueError("jpeg_optimize is for jpeg_frames: without them no JPEG is written")
    if jpeg_subsampling is not None:
        if jpeg_frames is None:
            raise ValueError("jpeg_subsampling is for jpeg_frames: without them no JPEG is written")
        from .jpeg import subsampling_value
        jpeg_subsampling = subsampling_value(jpeg_subsampling)
    if flow and "flow" not in _saved:
        from transflow.flow.sources.source import FlowSource as RefFlowSource
        _saved["flow"] = (RefFlowSource, RefFlowSource.__dict__["from_args"])
        RefFlowSource.from_args = _flow_from_args(RefFlowSource.from_args, horn_schunck, lucas_kanade, liteflownet,
                                                     motion_vectors, bool(device_flow_replay), bool(mjpeg_inputs),
                                                     bool(png_inputs), mjpeg_inputs == "parallel", yuv_inputs, yuv_input_matrix,
                                                     bool(resident_steps))
    if compositor and "compositor" not in _saved:
        from transflow.compositor.compositor import Compositor as RefCompositor

        from .compositor import bind_reference_data_layer
        bind_reference_data_layer()    # extra/control.py:155 asks isinstance(layer, DataLayer) of checkpointed layers
        _saved["compositor"] = (RefCompositor, RefCompositor.__dict__["from_args"])
        RefCompositor.from_args = _compositor_from_args(RefCompositor.from_args, lazy_frames, jpeg_frames,
                                                        "indexed" if png_frames == "indexed" else bool(png_frames), png_code,
                                                        bool(jpeg_optimize), jpeg_subsampling, yuv_frames, yuv_matrix, yuv_range,
                                                        reset_rng)
    if jpeg_frames is not None and "output" not in _saved:
        from transflow.output.video_output import VideoOutput as RefVideoOutput
        _saved["output"] = (RefVideoOutput, RefVideoOutput.__dict__["from_args"])
        RefVideoOutput.from_args = _output_from_args(RefVideoOutput.from_args, int(jpeg_frames), bool(jpeg_optimize),
                                                     2 if jpeg_subsampling is None else jpeg_subsampling)
    if png_frames and "output" not in _saved:
        from transflow.output.video_output import VideoOutput as RefVideoOutput
        _saved["output"] = (RefVideoOutput, RefVideoOutput.__dict__["from_args"])
        RefVideoOutput.from_args = _png_output_from_args(RefVideoOutput.from_args)
    if yuv_frames is not None and "output" not in _saved:
        from transflow.output.video_output import VideoOutput as RefVideoOutput
        _saved["output"] = (RefVideoOutput, RefVideoOutput.__dict__["from_args"])
        RefVideoOutput.from_args = _yuv_output_from_args(RefVideoOutput.from_args, yuv_frames, yuv_matrix, yuv_range)
    if device_flow_export and not _saved_export:
        import transflow.pipeline as ref_pipeline

        from . import deviceflow
        from .archive import DeviceFlowArchiveWriter
        _saved_export.append((ref_pipeline, ref_pipeline.NumpyOutput, deviceflow.DEVICE_ROUND))
        if device_flow_export == "indexed":
            import functools
            ref_pipeline.NumpyOutput = functools.partial(DeviceFlowArchiveWriter, index=True)
        else:
            ref_pipeline.NumpyOutput = DeviceFlowArchiveWriter
        deviceflow.DEVICE_ROUND = True
    if device_seam and not _saved_seam:
        import transflow.pipeline as ref_pipeline

        from . import deviceflow
        from .seam import FlowView
        merging = ref_pipeline.Pipeline.FLOW_MERGING_FUNCTIONS
        view = FlowView(lazy_frames=lazy_frames, jpeg_frames=jpeg_frames,
                        png_frames="indexed" if png_frames == "indexed" else bool(png_frames), png_code=png_code,
                        jpeg_optimize=bool(jpeg_optimize), jpeg_subsampling=jpeg_subsampling, yuv_frames=yuv_frames,
                        yuv_matrix=yuv_matrix, yuv_range=yuv_range)     # (its images are made at the first view)
        originals = (ref_pipeline.upscale_array, ref_pipeline.render1d, ref_pipeline.render2d, dict(merging))
        _saved_seam.append((ref_pipeline, *originals, deviceflow.DEVICE_VIEW, view))
        ref_pipeline.upscale_array, ref_pipeline.render1d, ref_pipeline.render2d, mergers = _seam_wrappers(originals, view)
        merging.update(mergers)         # in place: Pipeline.__init__ reads this dict
        deviceflow.DEVICE_VIEW = True
    if pixmaps or mjpeg_inputs or png_inputs or yuv_inputs:
        # one factory serves both options: a later call that asks for the other one adds it to what is installed
        from transflow.pixmap.source import PixmapSource as RefPixmapSource
        if "pixmaps" not in _saved:
            _saved["pixmaps"] = (RefPixmapSource, RefPixmapSource.__dict__["from_args"])
            _pixmap_options.update(stills=False, mjpeg=False, png=False, mjpeg_parallel=False, yuv=False, yuv_matrix="bt601")
        wanted = dict(stills=_pixmap_options["stills"] or bool(pixmaps), mjpeg=_pixmap_options["mjpeg"] or bool(mjpeg_inputs),
                      png=_pixmap_options["png"] or bool(png_inputs),
                      mjpeg_parallel=_pixmap_options["mjpeg_parallel"] or mjpeg_inputs == "parallel",
                      yuv=yuv_inputs or _pixmap_options["yuv"],
                      yuv_matrix=yuv_input_matrix if yuv_inputs else _pixmap_options["yuv_matrix"])
        if wanted != _pixmap_options:
            _pixmap_options.update(wanted)
            RefPixmapSource.from_args = _saved["pixmaps"][1]              # the reference's own, to be wrapped once
            RefPixmapSource.from_args = _pixmap_from_args(RefPixmapSource.from_args, wanted["stills"], wanted["mjpeg"],
                                                          wanted["png"], wanted["mjpeg_parallel"], wanted["yuv"],
                                                          wanted["yuv_matrix"])


def uninstall() -> None:
    for key in list(_saved):
        cls, original = _saved.pop(key)
        cls.from_args = original
    _pixmap_options.update(stills=False, mjpeg=False, png=False, mjpeg_parallel=False, yuv=False, yuv_matrix="bt601")
    while _saved_export:
        from . import deviceflow
        module, original, switch = _saved_export.pop()
        module.NumpyOutput = original
        deviceflow.DEVICE_ROUND = switch
    while _saved_seam:
        from . import deviceflow
        module, upscale_array, render1d, render2d, merging, switch, view = _saved_seam.pop()
        module.upscale_array, module.render1d, module.render2d = upscale_array, render1d, render2d
        module.Pipeline.FLOW_MERGING_FUNCTIONS.update(merging)
        deviceflow.DEVICE_VIEW = switch
        view.close()
