"""Drop-in mirror of ``rvc/scripts/audio_processing.py`` (the "processing" tab): ``convert_to_stereo`` -> ``add_effects`` ->
``combine_audio``, with the reference's positional signatures and return values.

The reference runs a pedalboard board one second at a time on the CPU and mixes with pydub.  Here the board is
``rvcx_fx_chain`` and the mix ``rvcx_op_fx_mix`` on the resident context (``infer/_state.py``); the arithmetic of every stage
is defined in include/rvcx.h ("post-production").  Neither pedalboard nor pydub is part of the reference tree: parity with
their classes is unpinned, the definitions are what is tested.  Files are read and written through ``infer/audio.py``: "wav"
and "flac" outputs work, any other ``output_format`` ("mp3", the tab's default, "m4a", ...) raises ``ValueError`` naming the
missing encoder before any work is done.  ``progress`` is accepted and ignored.

``process_audio_many(jobs)`` is new: a list of covers whose boards run in ONE ``rvcx_fx_chain`` call per (rate, settings).

Loudness (include/rvcx.h stages 9 - 12) is new as well.  ``measure_loudness(paths)`` reads LUFS and dBTP, one device call per
rate.  ``combine_audio``, ``process_audio`` and ``process_audio_many`` take the keyword-only ``target_lufs=None,
vocal_offset_lu=0.0, ceiling_dbtp=-1.0``: with ``target_lufs=None`` nothing changes (the int16 mix, byte for byte); with a
value the stems go through ``rvcx_fx_master`` as float -- both brought to the target, the vocal ``vocal_offset_lu`` above the
instrumental, the sum brought to the target again and limited to the ceiling.  The sliders ``vocal_gain`` /
``instrumental_gain`` are then added, in dB, to the computed gains; since the sum is normalised afterwards, what remains of
them is their difference, which moves the vocal against the instrumental.  ``last_master_report()`` returns the reports of
the last such call.

Key change (include/rvcx.h stages 13 and 14) is new too: the voice is transposed by ``pitch`` semitones in ``VC.pipeline``, the
instrumental stays in the old key.  ``shift_pitch(input_path, output_path, semitones)`` transposes a file at its length and
rate; the keyword-only ``instrumental_pitch=0.0`` of ``combine_audio``, ``process_audio`` and ``process_audio_many`` shifts the
instrumental on the device in front of the mix (back to int16 by clip(rint(32768 y)); with ``target_lufs`` the float result
goes to the master).  At 0.0 every file is byte for byte what it was.

Noise reduction (include/rvcx.h stage 15) is the "clean audio" switch of the UIs, which call noisereduce there: a soft spectral
gate on the device, this project's own definition (parity with noisereduce is unpinned).  ``reduce_noise(input_path,
output_path, strength)`` cleans a file at its length, rate and channel count, adaptively or from a noise clip
(``mode="profile", noise_path=...``); ``reduce_noise_many(jobs)`` runs one device call per (rate, channel count).  The
keyword-only ``vocal_denoise=0.0`` of ``process_audio`` and ``process_audio_many`` cleans the vocal in adaptive mode in front
of the board; at 0.0 every file is byte for byte what it was.

Formant shift (include/rvcx.h stages 17 and 18) is the "formant shifting" switch of the UIs: the spectral envelope of every
frame is estimated on the device and replaced by a warped copy.  ``shift_formants(input_path, output_path, semitones)`` moves
the formants of a file and leaves its pitch; ``shift_formants_many(jobs, semitones)`` runs one device call per (rate, channel
count); ``shift_pitch(..., preserve_formants=True)`` transposes a vocal stem and keeps its formants where they were.  The
keyword-only ``vocal_formant=0.0`` (semitones) of ``process_audio`` and ``process_audio_many`` shifts the formants of the vocal
behind ``vocal_denoise`` and in front of the board; at 0.0 every file is byte for byte what it was.
"""
from __future__ import annotations

import os
import tempfile

import numpy as np

from .. import _lib
from ..infer import _state
from ..infer.audio import convert_to_stereo, read_audio, write_output, write_wav_pcm16

__all__ = ["convert_to_stereo", "add_effects", "combine_audio", "process_audio", "process_audio_many", "measure_loudness",
           "last_master_report", "shift_pitch", "reduce_noise", "reduce_noise_many", "shift_formants", "shift_formants_many",
           "OUTPUT_DIR"]

OUTPUT_DIR = os.path.join(os.getcwd(), "output")

_FORMATS = ("wav", "flac")


def _check_format(output_format):
    if str(output_format).lower() not in _FORMATS:
        raise ValueError(f"output format {output_format!r}: this installation has no encoder for it (pydub's ffmpeg is not "
                         f"installed); the formats written here are {', '.join(_FORMATS)}")


def _stereo(a):
    """(frames,) or (frames, channels) -> (frames, 2): mono doubled, the first two channels otherwise"""
    a = np.asarray(a)
    if a.ndim == 1:
        return np.stack([a, a], axis=1)
    return np.ascontiguousarray(a[:, :2]) if a.shape[1] >= 2 else np.repeat(a, 2, axis=1)


def _pcm16(a):
    """read_audio's float64 -> the int16 samples pydub holds (a 16-bit file comes back exactly)"""
    return np.clip(np.rint(np.asarray(a, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _effects(ctx, signals, sr, values):
    """the board on a list of (frames, 2) float arrays of one rate and one setting: one rvcx_fx_chain call"""
    params = _lib.FxParams.make(values, sr, 2)
    with ctx.lock:
        return ctx.fx_chain([np.ascontiguousarray(_stereo(x), dtype=np.float32) for x in signals], params)


_reports = []


def last_master_report():
    """the reports of the last call that mastered (``target_lufs`` given), one dict per cover in the call's order: the keys
    of ``_lib.MASTER_REPORT`` and ``"path"``"""
    return [dict(r) for r in _reports]


def measure_loudness(path_or_paths):
    """-> [(LUFS, dBTP)] of one file or a list of files, as they are (mono or stereo); one rvcx_fx_loudness call per rate and
    channel count"""
    paths = [path_or_paths] if isinstance(path_or_paths, (str, os.PathLike)) else list(path_or_paths)
    ctx = _state.context()
    groups, out = {}, [None] * len(paths)
    for i, path in enumerate(paths):
        x, sr = read_audio(path)
        x = np.asarray(x, np.float32)
        x = x if x.ndim == 1 or x.shape[1] <= 2 else np.ascontiguousarray(x[:, :2])
        groups.setdefault((sr, 1 if x.ndim == 1 else x.shape[1]), []).append((i, x))
    for (sr, _), members in groups.items():
        with ctx.lock:
            got = ctx.fx_loudness([x for _, x in members], sr)
        for (i, _), r in zip(members, got):
            out[i] = r
    return out


def _shifted_many(ctx, items, sr, semitones):
    """a list of signals of one rate and channel count shifted by `semitones` in ONE rvcx_fx_pitch_shift call -> float32"""
    if not np.isfinite(semitones) or abs(semitones) > 12.0:
        raise ValueError(f"pitch shift of {semitones!r} semitones: a finite value within -12 .. 12 is expected")
    with ctx.lock:
        return ctx.fx_pitch_shift([np.ascontiguousarray(x, dtype=np.float32) for x in items], sr, float(semitones))


def _shifted(ctx, x, sr, semitones):
    """x (frames,) or (frames, 1 or 2) shifted by `semitones` on the device -> float32, x's shape"""
    return _shifted_many(ctx, [x], sr, semitones)[0]


def shift_pitch(input_path, output_path, semitones, *, preserve_formants=False):
    """The file transposed by `semitones` (-12 .. 12) at its own length, rate and channel count (more than two channels: the
    first two), written as 16-bit PCM through ``write_output``.  0 copies the samples.  ``preserve_formants``: the spectral
    envelope of the file is put back onto its transposed copy (include/rvcx.h stage 18) -- for a vocal stem, whose formants
    would otherwise move with the key."""
    x, sr = read_audio(input_path)
    x = np.asarray(x)
    x = x if x.ndim == 1 or x.shape[1] <= 2 else np.ascontiguousarray(x[:, :2])
    if semitones and preserve_formants:
        if not np.isfinite(semitones) or abs(semitones) > 12.0:
            raise ValueError(f"pitch shift of {semitones!r} semitones: a finite value within -12 .. 12 is expected")
        ctx = _state.context()
        with ctx.lock:
            y = ctx.fx_pitch_shift([np.ascontiguousarray(x, dtype=np.float32)], sr, float(semitones), preserve_formants=True)[0]
    else:
        y = _shifted(_state.context(), x, sr, semitones) if semitones else x
    write_output(output_path, _pcm16(y), sr)


def _two_channels(x):
    x = np.asarray(x)
    return x if x.ndim == 1 or x.shape[1] <= 2 else np.ascontiguousarray(x[:, :2])


_formant_params = _lib.formant_shift_params     # (sr, channels, semitones, quefrency_ms, amount): every refusal as ValueError


def _check_vocal_formant(vocal_formant):
    """``vocal_formant`` of process_audio(_many), before the first file is written: the default quefrency fits every rate, so
    the semitones are all there is to refuse"""
    _formant_params(16000, 2, vocal_formant)


def shift_formants_many(jobs, semitones, *, quefrency_ms=1.5, amount=1.0):
    """jobs: (input_path, output_path) tuples.  The formants of every file move by `semitones` (-12 .. 12; the pitch stays)
    through include/rvcx.h stage 17; every file keeps its length, rate and channel count (more than two channels: the first
    two) and is written as 16-bit PCM through ``write_output``; ONE rvcx_fx_formant call per (rate, channel count).  0
    semitones copies the samples.  Returns the output paths."""
    jobs = [tuple(j) for j in jobs]
    if any(len(j) != 2 for j in jobs):
        raise ValueError("shift_formants_many: a job is (input_path, output_path)")
    groups = {}
    for i, j in enumerate(jobs):
        x, sr = read_audio(j[0])
        x = np.asarray(_two_channels(x), np.float32)
        ch = 1 if x.ndim == 1 else x.shape[1]
        _formant_params(sr, ch, semitones, quefrency_ms, amount)     # every refusal before the first file is written
        groups.setdefault((sr, ch), []).append((i, x))
    ctx = _state.context() if semitones else None
    for (sr, ch), members in groups.items():
        if semitones:
            with ctx.lock:
                ys = ctx.fx_formant([x for _, x in members], sr, _formant_params(sr, ch, semitones, quefrency_ms, amount))
        else:
            ys = [x for _, x in members]
        for (i, _), y in zip(members, ys):
            write_output(jobs[i][1], _pcm16(y), sr)
    return [j[1] for j in jobs]


def shift_formants(input_path, output_path, semitones, *, quefrency_ms=1.5, amount=1.0):
    """The file with its formants moved by `semitones` (positive: brighter, a smaller vocal tract) and its pitch left alone,
    at its own length, rate and channel count, written as 16-bit PCM through ``write_output``.  ``quefrency_ms``: the
    resolution of the spectral envelope (lower it towards the period of a high voice); ``amount``: 0 .. 1."""
    shift_formants_many([(input_path, output_path)], semitones, quefrency_ms=quefrency_ms, amount=amount)


def _denoise_params(sr, channels, strength, mode, params):
    if mode not in _lib.FxDenoiseParams.MODES:
        raise ValueError(f"noise reduction mode {mode!r}: 'adaptive' or 'profile' is expected")
    if not (np.isfinite(strength) and 0.0 <= strength <= 1.0):
        raise ValueError(f"noise reduction strength {strength!r}: a value within 0 .. 1 is expected")
    try:
        p = _lib.FxDenoiseParams.make(sr, channels, mode=mode, strength=float(strength), **params)
        _lib.fx_denoise_host(np.zeros(1, np.float32), sr, p)         # the refusals of the library, on one sample of silence
    except _lib.RvcxError as e:
        raise ValueError(str(e)) from None
    return p


def _clip_for(noise_path, sr, channels):
    """the noise clip of a job as float32, at the item's rate and channel count"""
    if noise_path is None:
        return None
    z, sr_z = read_audio(noise_path)
    z = np.asarray(_two_channels(z), np.float32)
    if sr_z != sr or (1 if z.ndim == 1 else z.shape[1]) != channels:
        raise ValueError(f"noise clip {noise_path!r}: {sr_z} Hz, {1 if z.ndim == 1 else z.shape[1]} channel(s); the file to "
                         f"clean has {sr} Hz, {channels} channel(s)")
    return z


def reduce_noise_many(jobs, strength=0.7, *, mode="adaptive", noise_path=None, **params):
    """jobs: (input_path, output_path) or (input_path, output_path, noise_path) tuples; ``noise_path=`` is the clip of the
    jobs that name none (mode "profile" only; without any clip the file's own frames are the profile).  Every file keeps its
    length, rate and channel count (more than two channels: the first two) and is written as 16-bit PCM through
    ``write_output``; ONE rvcx_fx_denoise call per (rate, channel count).  ``params``: n_std, knee_db, thresh_mult, slope,
    time_constant_s, freq_smooth_hz, time_smooth_ms.  Strength 0 copies the samples.  Returns the output paths."""
    jobs = [tuple(j) for j in jobs]
    if any(len(j) not in (2, 3) for j in jobs):
        raise ValueError("reduce_noise_many: a job is (input_path, output_path) or (input_path, output_path, noise_path)")
    groups = {}
    for i, j in enumerate(jobs):
        x, sr = read_audio(j[0])
        x = np.asarray(_two_channels(x), np.float32)
        ch = 1 if x.ndim == 1 else x.shape[1]
        clip_path = j[2] if len(j) == 3 and j[2] is not None else noise_path
        if clip_path is not None and mode != "profile":
            raise ValueError("a noise clip needs mode='profile'")
        _denoise_params(sr, ch, strength, mode, params)              # every refusal before the first file is written
        groups.setdefault((sr, ch), []).append((i, x, _clip_for(clip_path, sr, ch)))
    ctx = _state.context() if strength else None
    for (sr, ch), members in groups.items():
        if strength:
            with ctx.lock:
                ys = ctx.fx_denoise([x for _, x, _ in members], sr, _denoise_params(sr, ch, strength, mode, params),
                                    noise=[z for _, _, z in members])
        else:
            ys = [x for _, x, _ in members]
        for (i, _, _), y in zip(members, ys):
            write_output(jobs[i][1], _pcm16(y), sr)
    return [j[1] for j in jobs]


def reduce_noise(input_path, output_path, strength=0.7, *, mode="adaptive", noise_path=None, **params):
    """The file cleaned by the spectral gate of include/rvcx.h stage 15 at its own length, rate and channel count, written as
    16-bit PCM through ``write_output``.  mode "adaptive" follows a noise floor per bin (a tone that holds steady for seconds
    becomes the floor and goes with it); mode "profile" takes its thresholds from ``noise_path``, a recording of the noise
    alone at the file's rate and channel count -- without one from the file's own frames, so that everything stationary in it
    counts as noise.  Strength 0 copies the samples."""
    reduce_noise_many([(input_path, output_path)], strength, mode=mode, noise_path=noise_path, **params)


def _stems(ctx, vocal_path, instrumental_path):
    """both files as float (frames, 2) at the vocal's rate"""
    v, sr = read_audio(vocal_path)
    m, sr_m = read_audio(instrumental_path)
    v, m = _stereo(v), _stereo(m)
    if sr_m != sr:
        with ctx.lock:
            m = np.stack([ctx.resample(m[:, c], sr_m, sr) for c in range(2)], axis=1)
    return v, m, sr


def _stems_many(ctx, pairs, instrumental_pitch=0.0):
    """[(vocal_path, instrumental_path)] -> [(v, m, sr)]; with ``instrumental_pitch`` the instrumentals of one rate are
    transposed in ONE rvcx_fx_pitch_shift call"""
    stems = [_stems(ctx, vp, ip) for vp, ip in pairs]
    if instrumental_pitch:
        rates = {}
        for k, (_, _, sr) in enumerate(stems):
            rates.setdefault(sr, []).append(k)
        for sr, members in rates.items():
            for k, m in zip(members, _shifted_many(ctx, [stems[k][1] for k in members], sr, instrumental_pitch)):
                stems[k] = (stems[k][0], m, sr)
    return stems


def _master(ctx, covers, target_lufs, vocal_offset_lu, ceiling_dbtp, instrumental_pitch=0.0):
    """covers: (vocal_path, instrumental_path, output_path, vocal_gain, instrumental_gain); one rvcx_fx_master call per
    (rate, slider difference)"""
    groups = {}
    stems = _stems_many(ctx, [(vp, ip) for vp, ip, _, _, _ in covers], instrumental_pitch)
    for k, ((_, _, op, gv, gi), (v, m, sr)) in enumerate(zip(covers, stems)):
        groups.setdefault((sr, float(gv) - float(gi)), []).append((k, op, np.asarray(v, np.float32), np.asarray(m, np.float32)))
    reports = [None] * len(covers)
    for (sr, slider), members in groups.items():
        with ctx.lock:
            outs, reps = ctx.fx_master([v for _, _, v, _ in members], [m for _, _, _, m in members], sr, target_lufs,
                                       vocal_offset_lu + slider, ceiling_dbtp)
        for (k, op, _, _), y, rep in zip(members, outs, reps):
            write_output(op, y, sr)
            reports[k] = dict(rep, path=op)
    _reports[:] = reports


def combine_audio(vocal_path, instrumental_path, output_path, vocal_gain, instrumental_gain, output_format, *,
                  target_lufs=None, vocal_offset_lu=0.0, ceiling_dbtp=-1.0, instrumental_pitch=0.0):
    """audio_processing.py:29-40: vocal + gain overlaid with instrumental + gain in int16, at the vocal's rate and length;
    with ``target_lufs`` the loudness-matched master of include/rvcx.h stage 12 instead; with ``instrumental_pitch`` the
    instrumental is transposed first (stage 14)"""
    _check_format(output_format)
    ctx = _state.context()
    if target_lufs is not None:
        _master(ctx, [(vocal_path, instrumental_path, output_path, vocal_gain, instrumental_gain)], target_lufs,
                vocal_offset_lu, ceiling_dbtp, instrumental_pitch)
        return
    v, sr = read_audio(vocal_path)
    m, sr_m = read_audio(instrumental_path)
    v, m = _stereo(v), _stereo(m)
    with ctx.lock:
        if sr_m != sr:
            m = np.stack([ctx.resample(m[:, c], sr_m, sr) for c in range(2)], axis=1)
        if instrumental_pitch:
            m = _shifted(ctx, m, sr, instrumental_pitch)
        out = ctx.fx_mix(_pcm16(v), _pcm16(m), vocal_gain, instrumental_gain)
    write_output(output_path, out, sr)       # FLAC for a path ending in ".flac", WAV bytes otherwise


def add_effects(vocal_path, output_path, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping, reverb_width,
                low_shelf_gain, high_shelf_gain, compressor_ratio, compressor_threshold, noise_gate_threshold,
                noise_gate_ratio, noise_gate_attack, noise_gate_release, chorus_rate_hz, chorus_depth,
                chorus_centre_delay_ms, chorus_feedback, chorus_mix):
    """audio_processing.py:54-109: the board on one file, written as a stereo 16-bit WAV"""
    values = (reverb_rm_size, reverb_wet, reverb_dry, reverb_damping, reverb_width, low_shelf_gain, high_shelf_gain,
              compressor_ratio, compressor_threshold, noise_gate_threshold, noise_gate_ratio, noise_gate_attack,
              noise_gate_release, chorus_rate_hz, chorus_depth, chorus_centre_delay_ms, chorus_feedback, chorus_mix)
    x, sr = read_audio(vocal_path)
    y = _effects(_state.context(), [x], sr, values)[0]
    write_wav_pcm16(output_path, y, sr)


def _check_paths(vocal_audio_path, instrumental_audio_path):
    if not vocal_audio_path:
        raise ValueError(
            "Не удалось найти аудиофайл с вокалом. "
            "Убедитесь, что файл загрузился или проверьте правильность пути к нему."
        )
    if not instrumental_audio_path:
        raise ValueError(
            "Не удалось найти аудиофайл с инструменталом. "
            "Убедитесь, что файл загрузился или проверьте правильность пути к нему."
        )


def process_audio(vocal_audio_path, instrumental_audio_path, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping,
                  reverb_width, low_shelf_gain, high_shelf_gain, compressor_ratio, compressor_threshold,
                  noise_gate_threshold, noise_gate_ratio, noise_gate_attack, noise_gate_release, chorus_rate_hz,
                  chorus_depth, chorus_centre_delay_ms, chorus_feedback, chorus_mix, output_format, vocal_gain,
                  instrumental_gain, use_effects, progress=None, *, target_lufs=None, vocal_offset_lu=0.0, ceiling_dbtp=-1.0,
                  instrumental_pitch=0.0, vocal_denoise=0.0, vocal_formant=0.0):
    """audio_processing.py:113-200 -> the path of the finished cover, OUTPUT_DIR/AiCover.<output_format>.  ``vocal_denoise``
    (0 .. 1): the stereo vocal is cleaned in adaptive mode (``reduce_noise``) in front of the board; ``vocal_formant``
    (semitones): its formants are moved (``shift_formants``) behind that and in front of the board"""
    _check_paths(vocal_audio_path, instrumental_audio_path)
    _check_format(output_format)
    _check_vocal_formant(vocal_formant)
    os.makedirs(OUTPUT_DIR, exist_ok=True)
    voice_stereo_path = os.path.join(OUTPUT_DIR, "Voice_Stereo.wav")
    aicover_path = os.path.join(OUTPUT_DIR, f"AiCover.{output_format}")
    if os.path.exists(aicover_path):
        os.remove(aicover_path)
    convert_to_stereo(vocal_audio_path, voice_stereo_path)
    if vocal_denoise:
        reduce_noise(voice_stereo_path, voice_stereo_path, vocal_denoise)
    if vocal_formant:
        shift_formants(voice_stereo_path, voice_stereo_path, vocal_formant)
    if use_effects:
        vocal_output_path = os.path.join(OUTPUT_DIR, "Vocal_Effected.wav")
        add_effects(voice_stereo_path, vocal_output_path, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping,
                    reverb_width, low_shelf_gain, high_shelf_gain, compressor_ratio, compressor_threshold,
                    noise_gate_threshold, noise_gate_ratio, noise_gate_attack, noise_gate_release, chorus_rate_hz,
                    chorus_depth, chorus_centre_delay_ms, chorus_feedback, chorus_mix)
    else:
        vocal_output_path = voice_stereo_path
    combine_audio(vocal_output_path, instrumental_audio_path, aicover_path, vocal_gain, instrumental_gain, output_format,
                  target_lufs=target_lufs, vocal_offset_lu=vocal_offset_lu, ceiling_dbtp=ceiling_dbtp,
                  instrumental_pitch=instrumental_pitch)
    return aicover_path


def process_audio_many(jobs, *, target_lufs=None, vocal_offset_lu=0.0, ceiling_dbtp=-1.0, instrumental_pitch=0.0,
                       vocal_denoise=0.0, vocal_formant=0.0):
    """A list of covers in one go.  Every job is the positional argument tuple of ``process_audio`` (24 values; a 25th, when
    given, is the output path -- the default is OUTPUT_DIR/AiCover_<index>.<output_format>).  The boards of all jobs that
    share a sample rate and the eighteen effect values run in ONE rvcx_fx_chain call; every cover is byte for byte what
    ``process_audio`` writes for the same arguments.  With ``target_lufs`` all covers of one rate (and one slider difference)
    are mastered in ONE rvcx_fx_master call.  ``instrumental_pitch`` transposes the instrumentals, all of one rate in ONE rvcx_fx_pitch_shift call.
    ``vocal_denoise`` cleans the stereo vocals in front of the boards, all of one rate in ONE rvcx_fx_denoise call;
    ``vocal_formant`` (semitones) then moves their formants, all of one rate in ONE rvcx_fx_formant call.  Returns the list of
    output paths."""
    jobs = [tuple(j) for j in jobs]
    for j in jobs:
        if len(j) not in (24, 25):
            raise ValueError("process_audio_many: a job is the 24 positional arguments of process_audio (+ an output path)")
        _check_paths(j[0], j[1])
        _check_format(j[20])
    _check_vocal_formant(vocal_formant)
    os.makedirs(OUTPUT_DIR, exist_ok=True)
    ctx = _state.context()
    outs = [j[24] if len(j) == 25 else os.path.join(OUTPUT_DIR, f"AiCover_{i}.{j[20]}") for i, j in enumerate(jobs)]
    with tempfile.TemporaryDirectory(prefix="rvcx_fx_") as tmp:
        vocal, groups = [], {}
        for i, j in enumerate(jobs):
            vocal.append(os.path.join(tmp, f"Voice_Stereo_{i}.wav"))
            convert_to_stereo(j[0], vocal[i])
        if vocal_denoise:
            reduce_noise_many([(v, v) for v in vocal], vocal_denoise)
        if vocal_formant:
            shift_formants_many([(v, v) for v in vocal], vocal_formant)
        for i, j in enumerate(jobs):
            if j[23]:
                x, sr = read_audio(vocal[i])
                groups.setdefault((sr, tuple(float(v) for v in j[2:20])), []).append((i, x))
        for (sr, values), members in groups.items():
            ys = _effects(ctx, [x for _, x in members], sr, values)
            for (i, _), y in zip(members, ys):
                vocal[i] = os.path.join(tmp, f"Vocal_Effected_{i}.wav")
                write_wav_pcm16(vocal[i], y, sr)
        for i, j in enumerate(jobs):
            if os.path.exists(outs[i]):
                os.remove(outs[i])
            if target_lufs is None and not instrumental_pitch:
                combine_audio(vocal[i], j[1], outs[i], j[21], j[22], j[20])
        if target_lufs is None and instrumental_pitch:      # the instrumentals of one rate in one call, then the int16 mixes
            stems = _stems_many(ctx, [(vocal[i], j[1]) for i, j in enumerate(jobs)], instrumental_pitch)
            for (i, j), (v, m, sr) in zip(enumerate(jobs), stems):
                with ctx.lock:
                    out = ctx.fx_mix(_pcm16(v), _pcm16(m), j[21], j[22])
                write_output(outs[i], out, sr)
        if target_lufs is not None:
            _master(ctx, [(vocal[i], j[1], outs[i], j[21], j[22]) for i, j in enumerate(jobs)], target_lufs, vocal_offset_lu,
                    ceiling_dbtp, instrumental_pitch)
    return outs
