"""Localisation overlays of a trained generator as PNG files: `python -m acimg.show video | images | boxes`.

Stands where the reference's three plotting scripts stand, with their flags, directories and file names:
* `video`: showvideo.py (records of `TFRecordDataLoader`): every frame's generated energy map over the grey frame,
  `<dir of train_file>/Generated_10s/I_%06d.png` (:63, :230).  No ffmpeg is run: `show.json` records the frame count, the
  12 fps rate, the file pattern and the two ffmpeg command lines of :247 and :260 as strings.  With `--avi 1` the merged
  clip of :260 is written as well, by this package: `<dir of train_file>/video_<class>_<video>_<checkpoint>.avi`, the
  frames as Motion-JPEG encoded on the device (`acimg.jpeg`: `acimg_jpeg_blocks`, `acimg_jpeg_scan`, `--quality`,
  `--restart_mcus`) and the records' sound as 16-bit PCM normalised to the clip's peak (`acimg.avi`), 1024 samples per
  frame at 12288 Hz; `show.json` then also names the file, its size, the quality, the restart interval and the rate;
* `images`: showimages.py: the real acoustic image's map beside the generated one's (real on the left, :107),
  `<checkpoint dir>/<model>_<data set>_AcousticMapJet_<checkpoint number>/<data set>_images_<n>.png` (:32-39, :151);
* `boxes`: showimages_bb.py with --plot 1 (box-annotated records, `BoxRecordLoader`): the generated map over the frame
  with the annotators' boxes outlined, `.../<model>_<data set>_AcousticFramesJet2_<n>/<data set>_images_<n>.png`
  (:40-47, :282).
All three build ResNet50Model + UNetAc(num_skip) and restore `--init_checkpoint` as `acimg.localize` does
(`build_trainer`), stream the data set through `Trainer.generate`, render on the device (`OverlayRenderer`:
`acimg_overlay_render`) and write with `acimg.png` (zlib only).  The pictures are the 224 x 298 frame itself, one
pixel per pixel: no figure margins, titles or resampling."""
import argparse
import json
import os
import sys

from .localize import build_trainer

RESULT_FILE = "show.json"
FPS = 12
SAMPLES_PER_FRAME = 1024
SAMPLE_RATE = SAMPLES_PER_FRAME * FPS      # 12288: sound and picture stay in step
GAP = 8      # white columns between the two panels of `images`

# showvideo.py:126-132: class directory -> the name in the merged video's file name
CLASS_NAMES = {
    "outdoor": dict(zip(("class_0", "class_1", "class_3", "class_5", "class_6", "class_7", "class_9"),
                        ("train", "boat", "fountain", "razor", "hairdryer", "hoover", "traffic"))),
    "old": dict(zip(("class_0", "class_1", "class_2", "class_3", "class_5", "class_6", "class_8", "class_10", "class_11"),
                    ("clapping", "fingersnapping", "speaking", "whistle", "clicking", "type", "hammering", "rippingpaper",
                     "plastic"))),
}


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m acimg.show", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--model", type=str, default="UNet", help="model type (UNet)")
        p.add_argument("--train_file", type=str, required=True, help="text file listing the TFRecord files")
        p.add_argument("--init_checkpoint", type=str, required=True, help="Saver-V2 checkpoint prefix (.../epoch_N.ckpt)")
        p.add_argument("--batch_size", type=int, default=2)
        p.add_argument("--sample_length", type=int, default=1, help="accepted as the scripts accept it; always 1 second")
        p.add_argument("--num_skip_conn", type=int, default=1, choices=(0, 1, 2))
        p.add_argument("--ae", type=int, default=0, help="1: plain auto-encoder generator (no sampling)")
        p.add_argument("--device", type=str, default="cuda:0")
        p.add_argument("--png_level", type=int, default=6, help="zlib level of the PNG files (0 - 9)")
        p.add_argument("--png_deflate", type=str, default="zlib", choices=("zlib", "device"),
                       help="device: the GPU deflates the PNG files' scanlines (acimg.deflate); --png_level is then unused")

    v = sub.add_parser("video", help="showvideo.py: the frames of a demo video")
    common(v)
    v.add_argument("--data_type", type=str, default="outdoor", help="outdoor or old: the class names of the video's name")
    v.add_argument("--avi", type=int, default=0, choices=(0, 1), help="1: also write the clip as MJPEG + PCM in an AVI file")
    v.add_argument("--quality", type=int, default=90, help="JPEG quality of the clip's frames (1 - 100)")
    v.add_argument("--restart_mcus", type=int, default=None,
                   help="16x16-pixel MCUs per JPEG restart interval (default: one MCU row)")
    i = sub.add_parser("images", help="showimages.py: real beside generated")
    common(i)
    i.add_argument("--datatype", type=str, default="outdoor")
    i.add_argument("--nr_frames", type=int, default=1)
    b = sub.add_parser("boxes", help="showimages_bb.py: generated map with the annotators' boxes")
    common(b)
    b.add_argument("--datatype", type=str, default="frames")
    b.add_argument("--nr_frames", type=int, default=1)
    b.add_argument("--plot", type=int, default=1)
    b.add_argument("--threshold", type=float, default=0.5)
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def dataset_name(args):
    return args.train_file.split("/")[-1].split(".")[0]


def checkpoint_number(args):
    base = args.init_checkpoint.split("/")[-1]
    parts = base.split("_")
    return (parts[1] if len(parts) > 1 else base).split(".ckpt")[0]


def output_dir(args):
    if args.command == "video":
        return "/".join(args.train_file.split("/")[:-1] + ["Generated_10s"])
    tag = "AcousticMapJet" if args.command == "images" else "AcousticFramesJet2"
    name = "{}_{}_{}_{}".format(args.model, dataset_name(args), tag, checkpoint_number(args))
    return "/".join(args.init_checkpoint.split("/")[:-1] + [name])


def file_pattern(args):
    """the file name of picture `num` as a Python format string"""
    return "I_{:06d}.png" if args.command == "video" else dataset_name(args) + "_images_{}.png"


def frame_file(args, num):
    return os.path.join(output_dir(args), file_pattern(args).format(num))


def merged_video_name(args):
    """showvideo.py:126-132, :260: video_<class name>_<video directory>_<checkpoint number>.avi"""
    parts = args.train_file.split("/")
    classe = parts[-3] if len(parts) >= 3 else ""
    videonum = parts[-2] if len(parts) >= 2 else ""
    label = CLASS_NAMES.get(args.data_type, CLASS_NAMES["old"]).get(classe, classe)
    return "video_{}_{}_{}.avi".format(label, videonum, checkpoint_number(args))


def avi_file(args):
    """the target of the merge command of `ffmpeg_commands`, unescaped: beside the train file, outside Generated_10s"""
    return "/".join(args.train_file.split("/")[:-1] + [merged_video_name(args)])


def ffmpeg_commands(args):
    """the two command lines showvideo.py:239-263 runs after the frames are saved (video track, then audio merge)"""
    parts = args.train_file.split("/")
    data_dir = "/".join(parts[:-1])
    esc = lambda s: s.replace(" ", "\\ ")  # noqa: E731
    video_file = "{}/video_track.avi".format(data_dir)
    track = "ffmpeg -y -r {} -f image2 -s 640x480 -i {}/Generated_10s/I_%06d.png -vcodec libx264 -crf 25 -pix_fmt yuv420p {}".format(
        FPS, esc(data_dir), esc(video_file))
    merge = "ffmpeg -y -i {} -i {} -codec copy -shortest {}/{}".format(
        esc(data_dir + "/audio/output_audio2.wav"), esc(video_file), esc(data_dir), merged_video_name(args))
    return [track, merge]


def write_avi(args, jpegs, samples, width, height=224):
    """the clip: one JPEG file and one [1024] row of `samples` (the clip's int32 audio) per frame -> summary entries"""
    from .avi import AviWriter, normalize_pcm
    pcm = normalize_pcm(samples).reshape(len(jpegs), SAMPLES_PER_FRAME)
    path = avi_file(args)
    with AviWriter(path, width, height, FPS, SAMPLE_RATE) as w:
        for jpeg, row in zip(jpegs, pcm):
            w.add_frame(jpeg, row)
    return dict(avi=path, avi_bytes=int(w.close()), sample_rate=SAMPLE_RATE)


def write_summary(args, num_frames, width, extra=None):
    d = output_dir(args)
    res = dict(command=args.command, num_frames=int(num_frames), file_pattern=file_pattern(args), directory=d,
               height=224, width=int(width), checkpoint=args.init_checkpoint)
    if args.command == "video":
        res.update(fps=FPS, printf_pattern="I_%06d.png", ffmpeg=ffmpeg_commands(args))
    res.update(extra or {})
    with open(os.path.join(d, RESULT_FILE), "w") as f:
        json.dump(res, f, indent=1)
    return res


def run(args, trainer=None, keep_energy=False, log=print):
    """render and save; returns the summary dict (+ 'energy': the generated images' [n,1728] float32 energy maps, and
    for `images` 'energy_real', as host arrays, when keep_energy)"""
    import numpy as np
    import torch

    from .data import BoxRecordLoader, TFRecordDataLoader
    from .evaluate import OverlayRenderer
    from .png import encode_png_many, write_png
    device = torch.device(args.device)
    tr = trainer if trainer is not None else build_trainer(args, device)
    avi = args.command == "video" and bool(args.avi)
    if args.command == "boxes":
        data = BoxRecordLoader(args.train_file, args.batch_size)
    else:
        # the video command reads audio + video alone (showvideo.py:72-75), so it plays converted recordings too
        data = TFRecordDataLoader(args.train_file, args.batch_size, device=device, raw_audio=avi,
                                  modalities=(1, 2) if args.command == "video" else None)
    rend = OverlayRenderer(device)
    deflater = None
    if args.png_deflate == "device":
        from .deflate import DeviceDeflater
        deflater = DeviceDeflater(device)
    if avi:      # the whole clip is kept (the sound's peak is known only at its end): a few MB for ten seconds
        from .jpeg import JpegEncoder
        enc, jpegs, sound = JpegEncoder(device, args.quality, args.restart_mcus), [], []
    os.makedirs(output_dir(args), exist_ok=True)
    num, width, kept, kept_real = 0, 298, [], []
    for batch in data.data:
        out = tr.generate(batch)
        energy = rend.energy(out)
        frames = batch[2].reshape(-1, 224, 298, 3)
        if args.command == "images":
            real = rend.energy(batch[0].reshape(-1, 36, 48, 12))
            img = rend.render_pair(frames, real, energy, gap=GAP)
            if keep_energy:
                kept_real.append(real.cpu().numpy())
        elif args.command == "boxes":
            img = rend.render(frames, energy, boxes=torch.stack(list(batch[3:7]), 1))
        else:
            img = rend.render(frames, energy)
        if keep_energy:
            kept.append(energy.cpu().numpy())
        if avi:
            jpegs.extend(enc.encode(img))
            sound.append(batch[6].numpy())
        width = int(img.shape[2])
        if deflater is not None:     # scanlines, Adler-32 and DEFLATE of the whole batch on the device: one call
            for data in encode_png_many(img, deflater):
                with open(frame_file(args, num), "wb") as f:
                    f.write(data)
                num += 1
        else:
            host = img.cpu().numpy()
            for h in range(host.shape[0]):
                write_png(frame_file(args, num), host[h], level=args.png_level)
                num += 1
        log("{} frames".format(num))
    if num == 0:
        raise ValueError("no samples in %s" % args.train_file)
    extra = None
    if avi:
        extra = write_avi(args, jpegs, np.concatenate(sound), width)
        extra.update(quality=enc.quality, restart_mcus=enc.restart_mcus(width))
    res = write_summary(args, num, width, extra=extra)
    if keep_energy:
        res["energy"] = np.concatenate(kept)
        if kept_real:
            res["energy_real"] = np.concatenate(kept_real)
    return res


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
