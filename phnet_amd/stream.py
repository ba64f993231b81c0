"""Streaming inference: one frame in, the lanes of that frame out, for B live video streams at once.

PHNet is an online detector - the only thing carried from frame to frame is the cross-frame memory (the tokens of the kept lanes
of the last `save_freq_max` frames).  `LaneStream` keeps that memory ON THE DEVICE as a token ring whose position is a word in
GPU memory (csrc/stream.hip), so that ONE captured hipGraph serves every frame of a video of any length: the first frames after
a reset, the frames after the ring has wrapped, one camera or several.  Per frame, on top of the T = 1 body of
`RouterOL.infer_clips_device`: one `stream_window` launch (the memory of all stages in logical order), one `stream_select` per
stage (streams without memory skip the cross-frame decoder, Router4OL.py:349-353) and one `stream_push` (the memory entry of
this frame for all stages); no `memory_tokens`, no `torch.cat` of the memory, no host round trip.

    s = model.open_stream(streams=B, frame_hw=(H, W))        # or LaneStream(model, streams=B, frame_hw=(H, W))
    s.reset()                                                # all streams; s.reset(mask) bool[B]: only those (a camera cut)
    rows, num, anchors = s.step(frames)                      # frames f32 [B,3,H,W]; device tensors, no host synchronisation
    lanes = s.lanes(rows, num)                               # list over streams of Lane lists

With `open_stream(..., polylines=True)` the step ends with one more launch (csrc/lane_points.hip) that leaves the lanes' (x, y)
points on the device in `s.polylines` (points, count, lanes_num, slot); `s.lanes_fast()` copies them to the host once and slices:

    lines = s.lanes_fast()                                   # list over streams of phnet_amd.polylines.Polyline lists

With `open_stream(..., track=True)` one launch after the decode (csrc/lane_track.hip, inside the captured graph, before the
polylines) gives every kept row an id that stays with the lane from frame to frame; `s.tracks` holds `track_id` and `hits`
(int32 [B,max_lanes], -1 / 0 where there is no lane) and `s.lanes_fast()` puts `track_id` into each polyline's metadata.

With `open_stream(..., polylines=True, render=LaneRenderer(...))` the step's last launch (csrc/lane_draw.hip) draws the lanes: a
label map and / or an overlay on the raw camera frame, in `s.rendered` (phnet_amd/overlay.py).

`LaneStreamV2` is the same for the Router4OLV2 family (what `Router4OLV2.RouterOL.open_stream` returns): there the decoder runs
for every stream and `stream_keys` (csrc/stream_v2.hip) picks each stream's key set - its memory window or its own tokens - from
the device-side frame count.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import hip_ops as K
from .graphed import warm_up


def window_order(n: int, W: int) -> List[int]:
    """Physical ring slots of the frames a stream remembers after n pushes since its reset, oldest first: with c = min(n, W),
    logical slot j < c is physical slot (n - c + j) % W (frame i was pushed to slot i % W).  The W - c empty slots are not listed:
    `stream_window` puts them LAST, masked - the attention kernel deals its keys round-robin to the lanes of a row and skips
    masked ones, so valid keys at unchanged positions followed by masked ones give the bits of the clip path's growing cat."""
    if n < 0 or W < 1:
        raise ValueError("window_order: n >= 0 and W >= 1")
    c = min(n, W)
    return [(n - c + j) % W for j in range(c)]


class StreamState:
    """Device state of B streams, allocated once: ring [S,B,W,L+1,E] / ring_valid bool [S,B,W,L+1] (the token ring; frame i of a
    stream lives in slot i % W), n int32 [B] (frames pushed since the stream's reset) and cursor int32 [B] (the copy of n that
    `stream_window` hands to `stream_push`: no launch reads the word it advances); plus the per-frame buffers window
    [S,B,W*(L+1),E], window_valid bool [S,B,W*(L+1)], has_memory bool [B] and feat [S,B,N,E] (this frame's attn feats).
    key_sets=True (the Router4OLV2 family) adds keys [B,Kmax,E] / keys_valid bool [B,Kmax], Kmax = max(N, W*(L+1)): the key set
    of the stage that is being decoded, rewritten by every stage's `stream_keys` launch; and no_anchors int64 [B,L], all -1 (the
    anchor list `push` takes when a frame leaves only its mean token in the memory)."""

    def __init__(self, stages: int, streams: int, slots: int, max_lanes: int, num_priors: int, width: int, device, key_sets: bool = False):
        S, B, W, L, N, E = stages, streams, slots, max_lanes, num_priors, width
        if min(S, B, W, L, N, E) < 1 or L >= N:
            raise ValueError("StreamState: positive sizes and max_lanes < num_priors expected")
        f32 = dict(dtype=torch.float32, device=device)
        self.ring = torch.zeros((S, B, W, L + 1, E), **f32)
        self.ring_valid = torch.zeros((S, B, W, L + 1), dtype=torch.bool, device=device)
        self.n = torch.zeros((B,), dtype=torch.int32, device=device)
        self.cursor = torch.zeros((B,), dtype=torch.int32, device=device)
        self.window = torch.zeros((S, B, W * (L + 1), E), **f32)
        self.window_valid = torch.zeros((S, B, W * (L + 1)), dtype=torch.bool, device=device)
        self.has_memory = torch.zeros((B,), dtype=torch.bool, device=device)
        self.feat = torch.zeros((S, B, N, E), **f32)
        if key_sets:                                              # Router4OLV2: the padded key set of one stage (hip_ops.stream_keys)
            self.keys = torch.zeros((B, max(N, W * (L + 1)), E), **f32)
            self.keys_valid = torch.zeros((B, max(N, W * (L + 1))), dtype=torch.bool, device=device)
            self.no_anchors = torch.full((B, L), -1, dtype=torch.int64, device=device)   # push list of the mean-token-only memory

    def load_window(self):
        K.stream_window(self.ring, self.ring_valid, self.n, self.cursor, out=(self.window, self.window_valid, self.has_memory))

    def push(self, anchors_sorted: torch.Tensor):
        K.stream_push(self.feat, anchors_sorted.contiguous(), self.ring, self.ring_valid, self.n, self.cursor)

    def reset(self, mask: Optional[torch.Tensor] = None):
        """n[b] = 0 for the chosen streams, in stream order.  Validity follows from n, so the ring is not cleared."""
        if mask is None:
            self.n.zero_()
        else:
            self.n.masked_fill_(mask, 0)


class LaneStream:
    """model: a RouterOL (eval).  streams: B.  frame_hw: (H, W) of the network input.  graph=True: the step is captured once
    (warmed up and captured the way GraphedInference does it) and replayed for every frame - a reset never recaptures;
    graph=False runs the same launches eagerly.  reset_every=k resets all streams before frames 0, k, 2k, ... (k = 16 is the
    chunking of the reference's testOL.py:104-117).  raw: a ClipPreprocessor - `step` then takes camera-format uint8 frames
    [B, *raw.frame_shape] (packed RGB [B,src_h,src_w,3], or the NV12 / YUYV surfaces of a ClipPreprocessor built with pixel_format=)
    and the colour conversion / crop / resize / normalise launch is part of the step (and of the captured graph).

    polylines=True: the last launch of the step (inside the captured graph) is `hip_ops.lane_points`; `polylines` then holds its
    four device tensors for the last step (points [B,max_lanes,S,2], count, lanes_num, slot) and `lanes_fast()` reads them.  What
    `step` returns does not change.

    track=True: the launch after the decode (inside the captured graph, before the polylines) is `hip_ops.lane_track` on a
    `tracking.TrackState` of max_tracks slots per stream (`track_state`); `tracks` = dict(track_id, hits), int32 [B,max_lanes],
    is written by every step.  max_tracks / max_age / match_thres (pixels of the network input): tracking.track_defaults.
    `reset(mask)` also frees the tracks of those streams (their next ids are new ones); `reset_every` resets the memory only -
    it is an evaluation protocol within one video, so ids carry across the chunk boundary.  Without track=True nothing is
    allocated, launched or returned differently.

    render: a phnet_amd.overlay.LaneRenderer (needs polylines=True) - the last launch of the step (inside the captured graph, after
    the polylines) is `hip_ops.lane_draw`; `rendered` = dict(label_map u8 [B,H,W] or None, overlay u8 [B,H,W,3] or None), allocated
    once and rewritten by every step.  Lanes are coloured by `tracks` with track=True, else by their index; an overlay is drawn on
    the raw camera frame when the stream has raw= (the renderer must take the same frames: LaneRenderer.for_preprocessor(raw)),
    else on black.  What `step` returns does not change; without render= nothing is allocated, launched or returned differently.

    With graph=True the returned tensors (and `polylines`, `tracks`, `rendered`) are the graph's static outputs: the next `step`
    overwrites them.

    precision: "fp32" (default) or "bf16" - the arithmetic of the step's conv / Linear GEMMs (INTEGRATION.md "bf16 inference"); the
    process-wide mode is what it was before, after the constructor and after every step."""

    def __init__(self, model, streams: int = 1, frame_hw: Tuple[int, int] = None, graph: bool = True, reset_every: Optional[int] = None,
                 raw=None, warmup: int = 2, polylines: bool = False, track: bool = False, max_tracks: Optional[int] = None,
                 max_age: Optional[int] = None, match_thres: Optional[float] = None, render=None, precision: str = "fp32"):
        K.precision_mode(precision, model.training)               # ValueError on an unknown name; "bf16" needs a model in eval()
        self.precision = precision
        if reset_every is not None and reset_every < 1:
            raise ValueError("reset_every must be a positive number of frames")
        if render is not None and not polylines:
            raise ValueError("render= draws the polylines: open the stream with polylines=True")
        if render is not None and render.overlay and raw is not None and tuple(render.frame_shape) != tuple(raw.frame_shape):
            raise ValueError(f"render= draws on {render.src_format} frames {tuple(render.frame_shape)}, raw= takes {tuple(raw.frame_shape)}")
        det = model.head
        if frame_hw is None:
            frame_hw = (det.img_h, det.img_w)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("LaneStream: the model must be on the GPU; phnet_amd has no CPU path")
        self.model, self.streams, self.reset_every, self.raw = model.eval(), int(streams), reset_every, raw
        self.want_polylines, self.polylines = bool(polylines), None
        self.state = self._new_state(det, dev)
        self.track_state, self.tracks = None, None
        if track:
            from .tracking import TrackState, track_defaults
            M, self.max_age, self.match_thr = track_defaults(model, max_tracks, max_age, match_thres)
            self.track_state = TrackState(self.streams, M, det.n_offsets, dev)
            self.tracks = {k: torch.zeros((self.streams, det.cfg.max_lanes), dtype=torch.int32, device=dev) for k in ("track_id", "hits")}
        if raw is not None:
            if (raw.out_h, raw.out_w) != tuple(frame_hw):
                raise ValueError(f"raw= resizes to {raw.out_h}x{raw.out_w}, frame_hw is {tuple(frame_hw)}")
            self.frames = torch.zeros((self.streams, *raw.frame_shape), dtype=torch.uint8, device=dev)
        else:
            self.frames = torch.zeros((self.streams, 3, *frame_hw), dtype=torch.float32, device=dev)
        self.render, self.rendered, self._step_frames = render, None, None
        if render is not None:
            render.prepare(dev)                                   # the palette's copy must not fall into the capture
            self.rendered = render.buffers((self.streams,), dev)
        self.frame_index = 0                                      # host-side count of steps, for reset_every only
        self.graph, self.out = None, None
        if graph:
            # the captured launches keep the arithmetic they were captured in, whatever the process mode is at replay
            with K.precision_scope(precision):
                warm_up(lambda: self._body(self.frames), warmup)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.out = self._body(self.frames)
            torch.cuda.synchronize()
        self.reset()                                              # the warm-up frames are forgotten
        if self.track_state is not None:
            self.track_state.next_id.fill_(1)                     # and so are the ids they used

    def _new_state(self, det, dev) -> StreamState:
        return StreamState(det.refine_layers, self.streams, self.model.save_freq_max, det.cfg.max_lanes, det.num_priors,
                           det.transformer_Dec.layers[0].self_attn.embed_dim, dev)

    @torch.no_grad()
    def _body(self, frames: torch.Tensor):
        """infer_clips_device's loop body for T = 1 on the B streams, the memory taken from / pushed to the device ring."""
        model, det, st = self.model, self.model.head, self.state
        model._begin_clip()
        self._step_frames = frames
        x = frames if self.raw is None else self.raw(frames)
        feats = model.backbone(x)
        front0 = det.stage0_front(feats[-1])
        st.load_window()
        outputs, _, gates = det.forward_clips(feats, None, front0, stream=st)
        dec = det.decode_frame(outputs, gates)
        st.push(dec["anchors_sorted"])
        model._begin_clip()
        return self._result(det, dec)

    def _result(self, det, dec):
        """What `step` returns; first, with track=True, the ids of this frame's lanes, with polylines=True their points and, with
        render=, the picture of them as the last launch of the step."""
        if self.track_state is not None:
            K.lane_track(dec["kept_rows"].contiguous(), dec["num"].contiguous(), self.track_state, self.match_thr, self.max_age,
                         out=self.tracks)
        if self.want_polylines:
            self.polylines, self._rows = det.points_device(dec), dec["kept_rows"]      # the rows `slot` points into
        if self.render is not None:                                                    # the step's last launch: the lanes on a picture
            self.render.render(self.polylines, frames=self._step_frames if self.raw is not None else None, tracks=self.tracks,
                               out=self.rendered)
        return dec["kept_rows"], dec["num"], dec["anchors"]

    def reset(self, mask=None):
        """Forget the memory of all streams, or of those where mask (bool [B]: tensor or sequence) is set - a camera cut.  The next
        frame of a reset stream is decoded like the first frame of a clip.  Stream-ordered, outside the graph: never recaptures."""
        if mask is not None and not torch.is_tensor(mask):
            mask = torch.tensor(list(mask), dtype=torch.bool)
        if mask is not None:
            if mask.dtype != torch.bool or mask.numel() != self.streams:
                raise ValueError(f"reset: bool mask of {self.streams} streams expected")
            mask = mask.reshape(-1).to(self.state.n.device, non_blocking=True)
        self.state.reset(mask)
        if self.track_state is not None:
            self.track_state.reset(mask)

    def step(self, frames: torch.Tensor):
        """One frame of every stream: frames f32 [B,3,H,W] (u8 [B, *raw.frame_shape] with raw=) on the device ->
        (kept_rows [B,max_lanes,6+S], num [B], anchors [B,max_lanes]) on the device.  No host synchronisation."""
        if frames.shape != self.frames.shape or frames.dtype != self.frames.dtype or not frames.is_cuda:
            raise ValueError(f"step: {self.frames.dtype} device frames {tuple(self.frames.shape)} expected, "
                             f"got {frames.dtype} {tuple(frames.shape)} on {frames.device}")
        if self.reset_every is not None and self.frame_index % self.reset_every == 0:
            self.state.reset()
        self.frame_index += 1
        if self.graph is None:
            with K.precision_scope(self.precision):
                return self._body(frames.contiguous())
        self.frames.copy_(frames, non_blocking=True)
        self.graph.replay()
        return self.out

    def lanes(self, kept_rows: torch.Tensor, num: torch.Tensor) -> Sequence[list]:
        """Device -> host copy of one step's result, then the host-side Lane construction: a list over streams of Lane lists."""
        return self.model.lanes_from_device(kept_rows, num)["lane_lines"]

    def lanes_fast(self) -> Sequence[list]:
        """The lanes of the last step from the device-side polylines: one device -> host copy, numpy slicing, no splines
        (phnet_amd.polylines.to_host).  A list over streams of Polyline lists, lane for lane the points of `lanes`; with
        track=True each Polyline's metadata carries its lane's "track_id"."""
        if self.polylines is None:
            raise RuntimeError("lanes_fast: open the stream with polylines=True and run a step first")
        from . import polylines as P
        return P.to_host(self.polylines["points"], self.polylines["count"], self.polylines["lanes_num"], self.polylines["slot"], self._rows,
                         track_id=None if self.tracks is None else self.tracks["track_id"])


class LaneStreamV2(LaneStream):
    """LaneStream for the Router4OLV2 family (libs.models.Router4OLV2.RouterOL): same constructor, same contract.  What differs
    per frame (DESIGN.md "Streaming path", V2 rules): the cross-frame decoder runs for EVERY stream, on a padded key set that
    `hip_ops.stream_keys` builds per stage - the stream's memory window from frame `cfg.save_freq` after its reset on, the
    frame's own tokens before - decided on the device from the frame count `stream_window` published; routing is hard
    (`route_lines`) over gates laid out [S, B*N]; and with `model.faithful_memory` the pushed memory entry is the one mean token
    of `saveMemory4Test` as shipped (an all -1 anchor list), otherwise the kept lanes' tokens + the mean of the rest (with
    graph=True the flag is read once, when the step is captured).  `gate_rows` [S, B*N] holds the gate scores the last step routed
    with (with graph=True the graph's static buffer, rewritten by the next step)."""

    def _new_state(self, det, dev) -> StreamState:
        return StreamState(det.refine_layers, self.streams, self.model.save_freq_max, det.cfg.max_lanes, det.num_priors,
                           det.reg_hidden_dim, dev, key_sets=True)

    @torch.no_grad()
    def _body(self, frames: torch.Tensor):
        """Router4OLV2.RouterOL.infer_clips_device's loop body for T = 1 on the B streams, keys and memory on the device."""
        model, det, st = self.model, self.model.head, self.state
        B, N = self.streams, det.num_priors
        self._step_frames = frames
        x = frames if self.raw is None else self.raw(frames)
        feats = model.backbone(x)
        gate_rows = torch.empty((det.refine_layers, B * N), dtype=torch.float32, device=x.device)
        front0 = det.stage0_front(feats[-1], gate_rows[0])
        st.load_window()
        outputs, _, _ = det.forward_clips(feats, None, front0, stream=st, gate_rows=gate_rows)
        dec = det.decode_frame(outputs, gate_rows, B)
        st.push(st.no_anchors if model.faithful_memory else dec["anchors_sorted"])
        self.gate_rows = gate_rows                                 # [S, B*N] of the last step (graph=True: the graph's static buffer)
        return self._result(det, dec)
