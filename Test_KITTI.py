#!/usr/bin/env python3
"""Inference / evaluation entry point (reference: Test_KITTI.py) on the MI355X implementation.

Two modes:
  * dataset mode (`-d <root> -tn Kitti2015`, `-tn Kitti_eigen_test_improved --test_list <file>`, or `-tn Kitti_eigen_test_original`, whose
    ground truth is the reference's `<frame>.npy` beside each image or -- `--velodyne-root <raw KITTI>` -- the frame's Velodyne scan
    projected on the GPU, fal_net_amd/velodyne.py): the reference's evaluation
    loop (Test_KITTI.py:103-117 file-list dataset at batch size 1, :163-208 forward + flip / multi-scale post-processing,
    :255-271 per-image KITTI depth errors and EPE, :277-280 `errors.txt`) over full-size frames of mixed sizes.  Frames are decoded
    by loader workers (Pillow) and normalised on the GPU; the network, `ms_pp` resampling and flips are HIP kernels; the metric
    chain is host-side numpy exactly as in the reference (fal_net_amd.myUtils), or -- `--device-metrics` -- HIP kernels that leave every
    frame's numbers in a device-resident table read once at the end (fal_net_amd/metrics.py).
  * `--synthetic`: seeded image of `--height x --width` (native KITTI 375x1242 by default), timing only -- no dataset on the box.
The command line is the reference's (Test_KITTI.py:36-60): `-m` is the model NAME and the checkpoint is <-dt>/<-ts>/<-m><-dtl>
(:119-120; `--checkpoint <file>` names it directly).  Image / PLY dumping (:211-253) is `--dump disp,input,pan,pc,feats` (any subset;
`--freeview V [--freeview-path orbit|dolly|pan]` adds V free-viewpoint views per frame, fal_net_amd/freeview.py, and `--freeview-fill [BETA]`
their hole-filled versions, fal_net_amd/inpaint.py;
`--sweep V [--sweep-range LO HI]` adds V views along the baseline and the right view's disparity, fal_net_amd/views.py;
`--stats KINDS` adds maps of the per-pixel disparity distribution (spread, entropy, arg-max plane, peak mass, peak disparity),
`--pc-min-conf C` keeps only the confident vertices of the point cloud and `--disparity peak` evaluates the peak disparity, fal_net_amd/confidence.py;
`--sparsification SCORES [--sparsification-steps S]` writes sparsification.txt: AUSE / AURG of the named confidence scores against the depth errors,
fal_net_amd/sparsification.py;
`--pseudo-lidar [--pl-beams N ...]` adds each frame's depth as a Velodyne-format scan Pseudo_lidar/<frame>.bin, fal_net_amd/pseudo_lidar.py;
`--mesh [--mesh-max-jump T ...]` adds each frame's depth as a triangle mesh Mesh/<frame>.ply, cut where depth jumps, fal_net_amd/mesh.py;
`--min-component K [--component-jump T]` drops from the mesh and the scan the pixels in connected pieces of the disparity map smaller than K pixels,
fal_net_amd/components.py;
`--cloud-metrics [--cm-thresholds T1,T2,... --cm-on gt|all --cm-beams N --cm-max-depth M]` writes cloud_errors.txt: Chamfer distance and F-score
between the back-projected prediction and ground truth, fal_net_amd/cloud_metrics.py;
fal_net_amd/dumps.py: the images, feature maps and point-cloud records are finished by HIP kernels, the host only encodes files); the
reference's `-save*` switches parse and are still refused when true.  `--dtype f16` is the recommended 16-bit
inference type (depth abs_rel vs the f32 path 2e-3, bf16 1.7e-2, at the same speed)."""
import argparse
import json
import os
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "5")  # application-level choice, before HIP initialises (fal_net_amd/__init__.py)

def _flag(v):
    """The reference declares its switches as untyped options with a default (`-fpp True`, `-eval False`, Test_KITTI.py:41-60), so the
    value arrives as a string; there every non-empty string -- 'False' included -- is truthy.  Here the words mean what they say."""
    if isinstance(v, bool):
        return v
    if str(v).strip().lower() in ('1', 'true', 't', 'yes', 'y', 'on'):
        return True
    if str(v).strip().lower() in ('0', 'false', 'f', 'no', 'n', 'off', ''):
        return False
    raise argparse.ArgumentTypeError('expected True or False, got {!r}'.format(v))


def _switch(p, *names, default, help):
    """`-name` alone, `-name True` and `-name False` all parse (the reference form is the one with a value)."""
    p.add_argument(*names, nargs='?', const=True, default=default, type=_flag, metavar='BOOL', help=help)


# The reference's command line (Test_KITTI.py:36-60): same flag names, meanings and defaults, except that --data has no default
# (the reference's is the author's desktop) and the values are typed.
parser = argparse.ArgumentParser(description='Testing pan generation (FAL_net on MI355X)', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('-d', '--data', metavar='DIR', default=None, help='path to dataset; frames are read from <data>/<tdataName>')
parser.add_argument('-tn', '--tdataName', metavar='Test Data Set Name', default='Kitti_eigen_test_improved',
                    choices=['Kitti2015', 'Kitti_eigen_test_improved', 'Kitti_eigen_test_original'])
parser.add_argument('-relbase', '--rel_baselne', type=float, default=1, help='Relative baseline of testing dataset')
parser.add_argument('-mdisp', '--max_disp', type=float, default=300, help='of the training patch W')
parser.add_argument('-mindisp', '--min_disp', type=float, default=2, help='of the training patch W')
parser.add_argument('-b', '--batch_size', metavar='Batch Size', type=int, default=1, help='accepted and set to 1 as the reference does (:112: KITTI mixes image sizes)')
_switch(parser, '-eval', '--evaluate', default=True, help='compute KITTI errors (+ EPE on Kitti2015) and write errors.txt')
_switch(parser, '-save', '--save', default=False, help='disparity PNG dumps (out of scope here: refused when true)')
_switch(parser, '-save_pc', '--save_pc', default=False, help='PLY point clouds (out of scope: refused when true)')
_switch(parser, '-save_pan', '--save_pan', default=False, help='synthesised views (out of scope: refused when true; crashes in the reference, :190)')
_switch(parser, '-save_input', '--save_input', default=False, help='input image dumps (out of scope: refused when true)')
parser.add_argument('-w', '--workers', metavar='Workers', type=int, default=4)
parser.add_argument('--sparse', default=False, action='store_true', help='Depth GT is sparse, automatically selected when choosing a KITTI dataset')
parser.add_argument('--print-freq', '-p', default=10, type=int, metavar='N', help='print frequency')
parser.add_argument('-gpu_no', '--gpu_no', default=None, help='GPU ID: exported as HIP_VISIBLE_DEVICES before HIP initialises (the reference sets '
                    "CUDA_VISIBLE_DEVICES, default '1'; here the default keeps the environment's device)")
parser.add_argument('-dt', '--dataset', help='Dataset and training stage directory', default='Kitti_stage2')
parser.add_argument('-ts', '--time_stamp', help='Model timestamp', default='10-18-15_42')
parser.add_argument('-m', '--model', help='Model name (FAL_netA / FAL_netB / FAL_netC); the checkpoint\'s own m_model entry wins, as in the reference (:122)', default='FAL_netB')
parser.add_argument('-no_levels', '--no_levels', type=int, default=49, help='Number of quantization levels in MED')
parser.add_argument('-dtl', '--details', help='details: the checkpoint is <dataset>/<time_stamp>/<model><details> (:119-120)', default=',e20es,b4,lr5e-05/checkpoint.pth.tar')
_switch(parser, '-fpp', '--f_post_process', default=False, help='Post-processing with flipped input')
_switch(parser, '-mspp', '--ms_post_process', default=True, help='Post-processing with multi-scale input')
_switch(parser, '-median', '--median', default=False, help='use median scaling (not needed when training from stereo)')
# additions of this implementation (no reference counterpart)
parser.add_argument('--checkpoint', default=None, help='checkpoint file given directly instead of composing it from -dt / -ts / -m / -dtl')
DEFAULT_TEST_LIST = os.path.join('Datasets', 'kitti_eigen_test_improved.txt')
ORIGINAL_TEST_LIST = os.path.join('Datasets', 'kitti_eigen_test_original.txt')
parser.add_argument('--test_list', default=DEFAULT_TEST_LIST,
                    help="Eigen split: one 'left right [gt]' line per frame, paths relative to <data>/<tdataName> (the reference opens "
                         "Datasets/kitti_eigen_test_improved.txt relative to the working directory); with -tn Kitti_eigen_test_original the "
                         "default becomes Datasets/kitti_eigen_test_original.txt")
parser.add_argument('--velodyne-root', default=None, metavar='DIR',
                    help='-tn Kitti_eigen_test_original: the raw KITTI tree (<DIR>/<date>/<drive>/velodyne_points/data/<frame>.bin and <DIR>/<date>/calib_*.txt); '
                         'every frame\'s ground truth is its Velodyne scan projected on the device (fal_net_amd/velodyne.py).  Default: the reference\'s layout, '
                         'a ready-made <frame>.npy depth map beside each image (tools/project_velodyne.py writes them)')
parser.add_argument('--velodyne-cam', type=int, default=2, choices=[2, 3], help='camera the scans are projected into (2: left colour image, 3: right)')
parser.add_argument('--save-path', default=None, help='where errors.txt / settings.txt go (default Test_Results/<tdataName>/<model>/<time_stamp>[fpp][mspp], :81-85)')
parser.add_argument('--synthetic', action='store_true', help='timing on a seeded image (default when no --data is given)')
parser.add_argument('--allow-seeded-weights', action='store_true', help='dataset mode without a checkpoint: evaluate SEEDED (untrained) weights (tests)')
parser.add_argument('--height', type=int, default=375)
parser.add_argument('--width', type=int, default=1242)
parser.add_argument('--iters', type=int, default=10)
parser.add_argument('--dtype', default='f16', choices=['f16', 'bf16', 'f32'])


def _comma_list(choices, message, strict):
    """argparse type of a comma-separated subset of `choices`, as a list in the order given.  strict: an empty list and a repeated name are
    refused as well.  message: the error's text, formatted with bad (the unknown names), choices and v (the value as given)."""
    def parse(v):
        names = [k for k in v.split(',') if k]
        bad = [k for k in names if k not in choices]
        if bad or (strict and (not names or len(set(names)) != len(names))):
            raise argparse.ArgumentTypeError(message.format(bad=','.join(bad), choices=','.join(choices), v=v))
        return names
    return parse


DUMP_KINDS = ('disp', 'input', 'pan', 'pc', 'feats')  # fal_net_amd/dumps.py: DUMP_KINDS
parser.add_argument('--dump', type=_comma_list(DUMP_KINDS, 'unknown dump kind(s) {bad}: choose from {choices}', strict=False), default=[], metavar='KINDS',
                    help='comma-separated subset of disp,input,pan,pc,feats: per-frame outputs of the reference\'s test script (:211-253) written under the '
                         'save path in its folders (l_disp, "Input im", Pan, Point_cloud, feats), finished on the GPU; --synthetic dumps its one frame')
parser.add_argument('--ply-format', default='binary', choices=['binary', 'ascii'], help='point clouds: binary_little_endian records, or the reference\'s ASCII file')
parser.add_argument('--device-percentile', action='store_true', help="ms_pp's 95th percentile from the exact device-side percentile kernel instead of the "
                    'copy to the host and np.percentile')
parser.add_argument('--device-metrics', action='store_true', help='KITTI depth errors (with -median too) and EPE from the device-side metric kernels '
                    '(fal_net_amd/metrics.py) into a table read once after the last frame, instead of two full-size copies and float64 numpy per frame')
parser.add_argument('--view-metrics', action='store_true',
                    help='also judge the synthesised right view against the real one: RMSE, MAE, PSNR and SSIM per frame from one more forward after the '
                         'timed region, on the device (fal_net_amd/metrics.py: view_errors, ssim); writes view_errors.txt and one JSON line.  --synthetic '
                         'has no real right image: the view is judged on a seeded stereo pair with known geometry (synthetic.structured_stereo)')


def write_view_errors(path, view):
    """view_errors.txt: the means over the frames of the synthesised view's errors against the real right image."""
    with open(path, 'w') as f:
        f.write('\nView synthesis over {} frames (8-bit units; SSIM: 11 x 11 Gaussian window, sigma 1.5)\n'.format(view['n']))
        f.write('\n' + ''.join('{:>10s}'.format(k) for k in ('rmse', 'mea', 'psnr', 'ssim')) + '\n')
        f.write(''.join('{:>10.4f}'.format(view[k]) for k in ('rmse', 'mea', 'psnr', 'ssim')) + '\n')


def _sweep_count(v):
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError('--sweep needs at least one view, got {}'.format(n))
    return n


parser.add_argument('--sweep', type=_sweep_count, default=None, metavar='V',
                    help='also render V views at evenly spaced fractions of the baseline over --sweep-range from each frame\'s logits (fal_net_amd/views.py: one '
                         'fused launch per 8 views) into Sweep/<frame>_v<view>.png, and the disparity in the right view\'s own frame into r_disp/<frame>.png')
parser.add_argument('--sweep-range', type=float, nargs=2, default=[-1.0, 1.0], metavar=('LO', 'HI'),
                    help='first and last baseline fraction of --sweep: 0 is the left camera, 1 the right one; |t| <= 2')


def _freeview_count(v):
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError('--freeview needs at least one pose, got {}'.format(n))
    return n


parser.add_argument('--freeview', type=_freeview_count, default=None, metavar='V',
                    help='also render V free-viewpoint views per frame along --freeview-path from the frame\'s logits (fal_net_amd/freeview.py: a homography '
                         'plane sweep, one launch per 8 poses, around the nominal camera of the frame\'s size) into Freeview/<frame>_p<pose>.png with the '
                         'coverage maps Freeview/<frame>_p<pose>_cover.png, and one JSON line with the mean cover')
parser.add_argument('--freeview-path', default='orbit', choices=['orbit', 'dolly', 'pan'],
                    help='--freeview: orbit circles the left camera in its image plane (radii X, Y of --freeview-amp, toed in by --freeview-yaw), dolly moves '
                         'forward from 0 to Z, pan turns on the spot from -DEG to DEG')
parser.add_argument('--freeview-amp', type=float, nargs=3, default=[0.5, 0.25, 0.5], metavar=('X', 'Y', 'Z'), help='--freeview: amplitudes of the path in baselines')
parser.add_argument('--freeview-yaw', type=float, default=3.0, metavar='DEG', help='--freeview: yaw amplitude of the path in degrees')
parser.add_argument('--freeview-fill', type=float, nargs='?', const=4.0, default=None, metavar='BETA',
                    help='--freeview: also fill the holes of every view from the background (fal_net_amd/inpaint.py: a pull-push pyramid biased towards '
                         'small disparity by BETA in [0, 8], 4 when the switch is given alone) into Freeview/<frame>_p<pose>_filled.png')
FREEVIEW_ARGS = ('freeview', 'freeview_path', 'freeview_amp', 'freeview_yaw')
FREEVIEW_FILL_ARGS = ('freeview_fill',)


def check_freeview_fill_args(a):
    """--freeview-fill belongs to --freeview, and its bias to [0, 8] (fal_net_amd/inpaint.py)."""
    if a.freeview_fill is None:
        return
    if a.freeview is None:
        raise SystemExit('--freeview-fill fills the holes of the --freeview views: give --freeview V as well')
    if not 0.0 <= a.freeview_fill <= 8.0:  # a NaN fails both comparisons
        raise SystemExit('--freeview-fill needs 0 <= BETA <= 8, got {}'.format(a.freeview_fill))


def freeview_poses(a):
    """The --freeview path as freeview.pose keyword sets (V of them), or None without --freeview."""
    if a.freeview is None:
        return None
    from fal_net_amd.freeview import paths
    x, y, z = a.freeview_amp
    if a.freeview_path == 'orbit':
        return paths.orbit(a.freeview, x, y, yaw=a.freeview_yaw)
    if a.freeview_path == 'dolly':
        return paths.dolly(a.freeview, 0.0, z)
    return paths.pan(a.freeview, -a.freeview_yaw, a.freeview_yaw)


STATS_KINDS = ('std', 'entropy', 'arg', 'conf', 'peak')


def _min_conf(name):
    def parse(v):
        from fal_net_amd.confidence import check_min_conf
        try:
            return check_min_conf(float(v), name)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))
    return parse


parser.add_argument('--stats', type=_comma_list(STATS_KINDS, '--stats takes a comma-separated subset of {choices} (each once), got {v!r}', strict=True),
                    default=None, metavar='KINDS',
                    help='comma-separated subset of std,entropy,arg,conf,peak: per-pixel statistics of each frame\'s distribution over the disparity planes '
                         '(fal_net_amd/confidence.py: one fused launch over the logits) as stats/<frame>_<kind>.png, and one JSON line with their means')
parser.add_argument('--pc-min-conf', type=_min_conf('--pc-min-conf'), default=None, metavar='C',
                    help='with --dump pc: Point_cloud/<frame>.ply holds only the vertices whose probability mass around the arg-max plane (conf) is at least C')
parser.add_argument('--disparity', default='mean', choices=['mean', 'peak'],
                    help='the disparity that is evaluated and dumped: the expectation over all planes, or the expectation over the arg-max plane and its '
                         'two neighbours of the same forward (only with -mspp False -fpp False)')


def _int_in(name, lo, hi):
    def parse(v):
        n = int(v)
        if not lo <= n <= hi:
            raise argparse.ArgumentTypeError('{} needs {} <= N <= {}, got {}'.format(name, lo, hi, v))
        return n
    return parse


def _positive(name):
    def parse(v):
        x = float(v)
        if not 0.0 < x < float('inf'):
            raise argparse.ArgumentTypeError('{} needs a finite positive number, got {}'.format(name, v))
        return x
    return parse


parser.add_argument('--pseudo-lidar', action='store_true',
                    help='also write each frame\'s depth as a Velodyne-format scan Pseudo_lidar/<frame>.bin (x forward, y left, z up, intensity 1 as float32: '
                         'what KITTI tools read), back-projected on the device (fal_net_amd/pseudo_lidar.py), and one JSON line with the point counts')
parser.add_argument('--pl-beams', type=_int_in('--pl-beams', 0, 128), default=0, metavar='N',
                    help='--pseudo-lidar: 0 keeps every valid pixel; N > 0 keeps the nearest point of each of N elevation x --pl-az-bins azimuth bins')
parser.add_argument('--pl-az-bins', type=_int_in('--pl-az-bins', 1, 4096), default=1024, metavar='N', help='--pseudo-lidar with --pl-beams: azimuth bins over -45..45 degrees')
parser.add_argument('--pl-max-depth', type=_positive('--pl-max-depth'), default=80.0, metavar='M', help='--pseudo-lidar: points beyond M metres are dropped')
parser.add_argument('--pl-max-height', type=float, default=1.0, metavar='M', help='--pseudo-lidar: points higher than M metres above the sensor are dropped (inf: none)')
parser.add_argument('--pl-min-conf', type=_min_conf('--pl-min-conf'), default=None, metavar='C',
                    help='--pseudo-lidar: keep only the pixels whose probability mass around the arg-max plane (conf) is at least C (one more forward per frame)')
parser.add_argument('--pl-calib', default=None, metavar='DIR',
                    help='--pseudo-lidar: directory holding calib_cam_to_cam.txt and calib_velo_to_cam.txt for every frame.  Default: each frame\'s own date with '
                         '-tn Kitti_eigen_test_original --velodyne-root, else a nominal pinhole camera at the image centre')
LIDAR_ARGS = ('pseudo_lidar', 'pl_beams', 'pl_az_bins', 'pl_max_depth', 'pl_max_height', 'pl_min_conf', 'pl_calib')


def _max_jump(v):
    x = float(v)
    if not x >= 0.0:
        raise argparse.ArgumentTypeError('--mesh-max-jump needs a number >= 0 (inf: no cut), got {}'.format(v))
    return x


def _mesh_max_depth(v):
    x = float(v)
    if not 0.0 < x < 200.0:
        raise argparse.ArgumentTypeError('--mesh-max-depth needs 0 < M < 200 (the point cloud caps depth at 200 m), got {}'.format(v))
    return x


parser.add_argument('--mesh', action='store_true',
                    help='also write each frame\'s depth as a triangle mesh Mesh/<frame>.ply: the pixel grid triangulated and cut where depth jumps, vertices and '
                         'faces compacted on the device (fal_net_amd/mesh.py), in the format of --ply-format, and one JSON line with the counts')
parser.add_argument('--mesh-max-jump', type=_max_jump, default=0.05, metavar='T',
                    help='--mesh: a triangle is cut when the depths of two of its vertices differ by more than the factor 1 + T (inf: only invalid vertices cut)')
parser.add_argument('--mesh-max-depth', type=_mesh_max_depth, default=80.0, metavar='M', help='--mesh: vertices beyond M metres are dropped')
parser.add_argument('--mesh-min-conf', type=_min_conf('--mesh-min-conf'), default=None, metavar='C',
                    help='--mesh: keep only the vertices whose probability mass around the arg-max plane (conf) is at least C (one more forward per frame)')
parser.add_argument('--mesh-normals', action='store_true', help='--mesh: per-vertex normals (nx ny nz) in the file, summed over the kept triangles around a vertex')
MESH_ARGS = ('mesh', 'mesh_max_jump', 'mesh_max_depth', 'mesh_min_conf', 'mesh_normals')


def _min_component(v):
    from fal_net_amd.components import check_min_component
    try:
        return check_min_component(int(v), '--min-component')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _component_jump(v):
    x = float(v)
    if not x >= 0.0:
        raise argparse.ArgumentTypeError('--component-jump needs a number >= 0 (inf: all valid neighbours joined), got {}'.format(v))
    return x


parser.add_argument('--min-component', type=_min_component, default=None, metavar='K',
                    help='--mesh / --pseudo-lidar: a speckle filter -- keep only the pixels whose connected component of the disparity map (4-neighbours '
                         'joined where the disparities differ by at most the factor 1 + --component-jump; fal_net_amd/components.py, labelled on the device) '
                         'holds at least K pixels, and one JSON line with the component counts')
parser.add_argument('--component-jump', type=_component_jump, default=None, metavar='T',
                    help='--min-component: two neighbours belong together when their disparities differ by at most the factor 1 + T (default: '
                         '--mesh-max-jump for the mesh, 0.05 for the scan)')
COMPONENT_ARGS = ('min_component', 'component_jump')


SPARSIFICATION_SCORES = ('std', 'entropy', 'conf', 'relstd')  # fal_net_amd/sparsification.py: SCORES

parser.add_argument('--sparsification', type=_comma_list(SPARSIFICATION_SCORES, '--sparsification takes a comma-separated subset of {choices} (each once), got {v!r}',
                                                         strict=True), default=None, metavar='SCORES',
                    help='comma-separated subset of std,entropy,conf,relstd: per frame with ground truth, remove the pixels in order of each score and of the true '
                         'error and recompute abs_rel, rms and d1 = 1 - a1 on the rest (fal_net_amd/sparsification.py: sorted and summed on the device); writes '
                         'sparsification.txt with AUSE and AURG per score and the mean curves, and one JSON line.  Dataset mode with -eval True only')
parser.add_argument('--sparsification-steps', type=_int_in('--sparsification-steps', 2, 100), default=None, metavar='S',
                    help='--sparsification: the number of cuts of every curve; cut j removes the j / S most uncertain pixels (default 50)')
SPARSIFICATION_ARGS = ('sparsification', 'sparsification_steps')


SWEEP_ARGS = ('sweep', 'sweep_range')
STATS_ARGS = ('stats', 'pc_min_conf', 'disparity')
# One row per family of switches: (the switch, the family's names in settings.txt with the switch's own first, is the family on?, are its
# parameters refused without the switch?).  The --stats family has three switches of equal standing and no parameters.
FAMILIES = (
    ('--sweep', SWEEP_ARGS, lambda a: a.sweep is not None, False),
    ('--stats', STATS_ARGS, lambda a: a.stats is not None or a.pc_min_conf is not None or a.disparity != 'mean', False),
    ('--pseudo-lidar', LIDAR_ARGS, lambda a: a.pseudo_lidar, True),
    ('--mesh', MESH_ARGS, lambda a: a.mesh, True),
    ('--sparsification', SPARSIFICATION_ARGS, lambda a: a.sparsification is not None, True),
    ('--freeview', FREEVIEW_ARGS, lambda a: a.freeview is not None, False),
    ('--freeview-fill', FREEVIEW_FILL_ARGS, lambda a: a.freeview_fill is not None, False),
)


def hidden_settings(a):
    """The names settings.txt leaves out: those of every family that is off, so that a run without a family writes the file it wrote before the
    family existed."""
    return tuple(n for _, names, on, _ in FAMILIES if not on(a) for n in names)


# Families added after hidden_settings() was pinned to the table above: the same four-tuples, walked after FAMILIES by check_family_args and by the
# settings.txt filter (settings_hidden)
LATER_FAMILIES = (
    ('--min-component', COMPONENT_ARGS, lambda a: a.min_component is not None, True),
)


def settings_hidden(a):
    """What settings.txt leaves out: hidden_settings, then the names of every later family that is off."""
    return hidden_settings(a) + tuple(n for _, names, on, _ in LATER_FAMILIES if not on(a) for n in names)


def _cm_thresholds(v):
    from fal_net_amd.cloud_metrics import check_thresholds
    try:
        return list(check_thresholds([float(x) for x in v.split(',') if x]))
    except ValueError as e:
        raise argparse.ArgumentTypeError('--cm-thresholds: {}'.format(e))


parser.add_argument('--cloud-metrics', action='store_true',
                    help='also score each frame in 3-D: the predicted depth back-projected into a point cloud against the back-projected ground truth -- '
                         'accuracy, completeness and Chamfer distance in metres, precision / recall / F-score at --cm-thresholds -- by an all-pairs nearest-'
                         'neighbour kernel on the device (fal_net_amd/cloud_metrics.py); writes cloud_errors.txt and one JSON line.  Dataset mode with '
                         '-eval True only; the calibration is --pseudo-lidar\'s (--pl-calib, the frame\'s own, or a nominal camera)')
parser.add_argument('--cm-thresholds', type=_cm_thresholds, default=None, metavar='T1,T2,...',
                    help='--cloud-metrics: up to 8 increasing distance thresholds of the F-score in metres (default 0.1,0.25,0.5,1.0)')
parser.add_argument('--cm-on', default='gt', choices=['gt', 'all'],
                    help='--cloud-metrics: the predicted cloud holds only the pixels that carry ground truth (gt), or every pixel (all)')
parser.add_argument('--cm-beams', type=_int_in('--cm-beams', 0, 128), default=0, metavar='N',
                    help='--cloud-metrics: N > 0 first reduces the predicted cloud to the nearest point of each of N elevation x 1024 azimuth bins')
parser.add_argument('--cm-max-depth', type=_positive('--cm-max-depth'), default=80.0, metavar='M', help='--cloud-metrics: points of either cloud beyond M metres are dropped')
CLOUD_ARGS = ('cloud_metrics', 'cm_thresholds', 'cm_on', 'cm_beams', 'cm_max_depth')
# Families added after settings_hidden() was pinned to the two tables above: the same four-tuples again, walked after LATER_FAMILIES by
# check_family_args and by the settings.txt filter (settings_left_out)
NEWER_FAMILIES = (
    ('--cloud-metrics', CLOUD_ARGS, lambda a: a.cloud_metrics, True),
)
LATER_LINE_ORDER = ('cloud',)  # the JSON lines printed after LINE_ORDER's


def settings_left_out(a):
    """What settings.txt leaves out: settings_hidden, then the names of every newer family that is off."""
    return settings_hidden(a) + tuple(n for _, names, on, _ in NEWER_FAMILIES if not on(a) for n in names)


def _ground_arg(name, key, cast):
    """argparse type of one --ground-* parameter: the range check is ground.check_fit_args's."""
    def parse(v):
        from fal_net_amd.ground import check_fit_args
        try:
            return check_fit_args(**{key: cast(v)})[key]
        except ValueError as e:
            raise argparse.ArgumentTypeError('{}: {}'.format(name, e))
    return parse


def _remove_ground(v):
    x = float(v)
    if not -float('inf') < x < float('inf'):
        raise argparse.ArgumentTypeError('--pl-remove-ground needs a finite height in metres, got {}'.format(v))
    return x


parser.add_argument('--ground', action='store_true',
                    help='also fit each frame\'s road plane: the depth back-projected densely (no height ceiling, within --pl-max-depth), plane hypotheses '
                         'through seeded point triples scored by their inlier count in an all-pairs kernel on the device, the winner refitted from the '
                         'moments of its inliers (fal_net_amd/ground.py); writes Ground/<frame>.txt in the KITTI-object planes format (camera axes) and one '
                         'JSON line with the mean camera height, tilt, inlier fraction and rms; the calibration is --pseudo-lidar\'s')
parser.add_argument('--ground-tol', type=_ground_arg('--ground-tol', 'tol', float), default=0.15, metavar='M',
                    help='--ground / --pl-remove-ground: a point within M metres of a plane, vertically, is its inlier')
parser.add_argument('--ground-hypotheses', type=_ground_arg('--ground-hypotheses', 'hypotheses', int), default=512, metavar='N',
                    help='--ground / --pl-remove-ground: the number of plane hypotheses, 1 to 4096')
parser.add_argument('--ground-seed', type=int, default=0, metavar='S', help='--ground / --pl-remove-ground: the seed of the hypotheses\' point triples')
parser.add_argument('--ground-max-tilt', type=_ground_arg('--ground-max-tilt', 'max_tilt', float), default=15.0, metavar='DEG',
                    help='--ground / --pl-remove-ground: hypotheses tilted more than DEG degrees against the sensor\'s horizontal are left out')
parser.add_argument('--ground-refits', type=_ground_arg('--ground-refits', 'refits', int), default=2, metavar='K',
                    help='--ground / --pl-remove-ground: the plane is refitted K >= 1 times from the moments of its inliers')
parser.add_argument('--pl-remove-ground', type=_remove_ground, nargs='?', const=0.2, default=None, metavar='H',
                    help='--pseudo-lidar: take the ground out of the scan -- every point at most H metres (0.2 when the switch is given alone) above the '
                         'frame\'s fitted road plane is dropped; a frame without a plane is written unfiltered and counted')
GROUND_ARGS = ('ground', 'ground_tol', 'ground_hypotheses', 'ground_seed', 'ground_max_tilt', 'ground_refits')
REMOVE_GROUND_ARGS = ('pl_remove_ground',)
# Families added after settings_left_out() was pinned to the three tables above: the same four-tuples once more, walked after NEWER_FAMILIES by
# check_family_args and by the settings.txt filter (settings_omitted).  The --ground-* parameters belong to both switches.
GROUND_FAMILIES = (
    ('--ground', GROUND_ARGS, lambda a: a.ground or a.pl_remove_ground is not None, True),
    ('--pl-remove-ground', REMOVE_GROUND_ARGS, lambda a: a.pl_remove_ground is not None, False),
)
GROUND_LINE_ORDER = ('ground',)  # the JSON lines printed after LATER_LINE_ORDER's


def ground_left_out(a):
    """The names of every ground family that is off: what settings.txt leaves out besides settings_left_out."""
    return tuple(n for _, names, on, _ in GROUND_FAMILIES if not on(a) for n in names)


def settings_omitted(a):
    """Everything settings.txt leaves out: settings_left_out, then ground_left_out."""
    return settings_left_out(a) + ground_left_out(a)


def check_ground_args(a):
    """--pl-remove-ground filters the scan of --pseudo-lidar.  SystemExit says so."""
    if a.pl_remove_ground is not None and not a.pseudo_lidar:
        raise SystemExit('--pl-remove-ground takes the ground out of the scan of --pseudo-lidar: add --pseudo-lidar')


def ground_fit_args(a):
    """The --ground-* parameters as the keywords of ground.fit."""
    return dict(tol=a.ground_tol, hypotheses=a.ground_hypotheses, seed=a.ground_seed, max_tilt=a.ground_max_tilt, refits=a.ground_refits)


def check_cloud_args(a, dataset_mode):
    """--cloud-metrics needs ground truth.  SystemExit says which."""
    if not a.cloud_metrics:
        return
    if not dataset_mode:
        raise SystemExit('--cloud-metrics compares the predicted cloud with the ground truth\'s, and synthetic mode has no ground truth: give a dataset (-d <root>)')
    if not a.evaluate:
        raise SystemExit('--cloud-metrics needs the ground truth: run with -eval True')


def write_cloud_errors(path, res):
    """cloud_errors.txt: the means over the counted frames, then one line per frame."""
    K = range(len(res['thresholds']))
    head = ['accuracy', 'completeness', 'chamfer', 'chamfer_l2'] + ['{}@{:g}'.format(k, t) for t in res['thresholds'] for k in ('P', 'R', 'F')]

    def line(acc, comp, ch, ch2, P, R, F):
        return ''.join('{:>14.6f}'.format(v) for v in [acc, comp, ch, ch2] + [x[k] for k in K for x in (P, R, F)])

    with open(path, 'w') as f:
        f.write('Cloud metrics over {} frames (distances in metres between the back-projected prediction and ground truth; accuracy: prediction -> '
                'ground truth, completeness: ground truth -> prediction, chamfer: their sum, chamfer_l2: the same of the squared distances; '
                'P / R / F at each threshold)\n'.format(res['frames']))
        f.write('{:>8s}{:>10s}{:>10s}'.format('frame', 'n_pred', 'n_gt') + ''.join('{:>14s}'.format(h) for h in head) + '\n')
        f.write('{:>8s}{:>10.1f}{:>10.1f}'.format('mean', res['n_pred_mean'], res['n_gt_mean']) + line(*(res[k + '_mean'] for k in (
            'accuracy', 'completeness', 'chamfer', 'chamfer_l2', 'precision', 'recall', 'f'))) + '\n')
        for i in range(len(res['rows'])):
            f.write('{:>8d}{:>10.0f}{:>10.0f}'.format(i, res['n_pred'][i], res['n_gt'][i]) + line(*(res[k][i] for k in (
                'accuracy', 'completeness', 'chamfer', 'chamfer_l2', 'precision', 'recall', 'f'))) + '\n')


def check_component_args(a):
    """--min-component filters the products that have pixels to drop; SystemExit names them when neither is on."""
    if a.min_component is not None and not (a.mesh or a.pseudo_lidar):
        raise SystemExit('--min-component filters the products of --mesh and --pseudo-lidar: add --mesh or --pseudo-lidar')


def check_family_args(a):
    """A family's parameters change nothing without its switch: SystemExit names the ones that were given (the families whose parameters are
    refused; --sweep-range and the --freeview path parameters are accepted in silence)."""
    for switch, names, on, strict in FAMILIES + LATER_FAMILIES + NEWER_FAMILIES + GROUND_FAMILIES:
        given = [] if on(a) or not strict else [n for n in names[1:] if getattr(a, n) != parser.get_default(n)]
        if given:
            raise SystemExit('{} {} a parameter of {}: add {}'.format(', '.join('--' + n.replace('_', '-') for n in given),
                                                                       'sets' if len(names) == 2 else 'set(s)', switch, switch))
    if a.pseudo_lidar and a.pl_max_height != a.pl_max_height:
        raise SystemExit('--pl-max-height is not a number')


def check_sparsification_args(a, dataset_mode):
    """--sparsification needs ground truth.  SystemExit says which."""
    if a.sparsification is None:
        return
    if not dataset_mode:
        raise SystemExit('--sparsification compares the scores with the depth errors, and synthetic mode has no ground truth: give a dataset (-d <root>)')
    if not a.evaluate:
        raise SystemExit('--sparsification needs the depth errors: run with -eval True')


def write_sparsification(path, res):
    """sparsification.txt: one line per score with AUSE and AURG of the three metrics (means over the frames with ground truth), then the mean curves."""
    with open(path, 'w') as f:
        f.write('Sparsification over {} frames, {} cuts (AUSE: area between score and oracle, lower is better; AURG: area between random and score, '
                'higher is better)\n'.format(res['frames'], res['steps']))
        for k in res['names']:
            f.write('{:>8s}: '.format(k) + '  '.join('ause_{0} {1:.6f} aurg_{0} {2:.6f}'.format(m, res['ause_mean'][k][m], res['aurg_mean'][k][m])
                                                    for m in res['metrics']) + '\n')
        f.write('\nMean curves (fraction removed: 0, 1/S, ..., (S-1)/S)\n')
        for m in res['metrics']:
            f.write('{:>8s} {:>8s}: '.format('oracle', m) + ' '.join('{:.6f}'.format(v) for v in res['oracle_mean'][m]) + '\n')
            for k in res['names']:
                f.write('{:>8s} {:>8s}: '.format(k, m) + ' '.join('{:.6f}'.format(v) for v in res['curves_mean'][k][m]) + '\n')


def nominal_calibration(H, W):
    """(P, fb) of a frame without calibration files: velodyne.nominal_matrix with the focal length of myUtils.width_to_focal and
    metrics.focal_baseline('eigen', W); a width that is no KITTI width has neither, and takes the 1242-pixel camera scaled to it (dumps.camera_for_width)."""
    from fal_net_amd import dumps, metrics, velodyne
    from fal_net_amd.myUtils import width_to_focal
    if W in width_to_focal:
        focal, fb = width_to_focal[W], metrics.focal_baseline('eigen', W)
    else:
        focal, baseline = dumps.camera_for_width(W)
        fb = focal * baseline
    return velodyne.nominal_matrix(H, W, focal), fb


def lidar_calibration(a, triples=None):
    """Where --pseudo-lidar takes P and fb from -> (callable (frame index, H, W) -> (P, fb), a word for the output): --pl-calib DIR for every frame;
    each frame's own date where the triples carry a calibration directory (the original split with --velodyne-root); else the nominal camera."""
    from fal_net_amd import velodyne
    cache = {}

    def from_dir(d):
        if d not in cache:
            cache[d] = (velodyne.projection_matrix(d, a.velodyne_cam), velodyne.focal_baseline(d, a.velodyne_cam))
        return cache[d]

    if a.pl_calib is not None:
        from_dir(a.pl_calib)  # a missing file stops the run here, not after the first forward
        return (lambda i, H, W: from_dir(a.pl_calib)), 'pl-calib'
    if triples and all(hasattr(t[2], 'calib_dir') for t in triples):
        return (lambda i, H, W: from_dir(triples[i][2].calib_dir)), 'frame'
    return (lambda i, H, W: nominal_calibration(H, W)), 'nominal'


def check_confidence_args(a):
    """What the confidence switches need of the others; SystemExit names what is missing."""
    if a.pc_min_conf is not None and 'pc' not in a.dump:
        raise SystemExit('--pc-min-conf filters the point cloud of --dump pc: add pc to --dump')
    if a.disparity == 'peak' and (a.f_post_process or a.ms_post_process):
        raise SystemExit('--disparity peak is valid only with both post-processing modes off (-mspp False -fpp False): ms_pp and the flip '
                         'post-processing blend two expectation maps and are not redefined for the peak disparity')


def checkpoint_path(a):
    """Test_KITTI.py:119-120: os.path.join(args.dataset, args.time_stamp, args.model + args.details); --checkpoint overrides."""
    return a.checkpoint or os.path.join(a.dataset, a.time_stamp, a.model + a.details)


def resolve_test_list(a):
    """--test_list; left at its default with -tn Kitti_eigen_test_original it is that split's own list (Kitti_eigen_test_original.py:32)."""
    if a.tdataName == 'Kitti_eigen_test_original' and a.test_list == DEFAULT_TEST_LIST:
        return ORIGINAL_TEST_LIST
    return a.test_list


def sweep_fractions(a):
    """The --sweep baseline fractions: V evenly spaced values from LO to HI (one view: LO), or None without --sweep."""
    if a.sweep is None:
        return None
    lo, hi = a.sweep_range
    return [lo + (hi - lo) * i / (a.sweep - 1) for i in range(a.sweep)] if a.sweep > 1 else [lo]


def refuse_out_of_scope(a):
    on = [n for n in ('save', 'save_pc', 'save_pan', 'save_input') if getattr(a, n)]
    if on:
        raise SystemExit('{}: image / point-cloud dumps (reference Test_KITTI.py:211-253) are out of scope of this implementation; '
                         'run without them to evaluate'.format(', '.join('-' + n for n in on)))


LINE_ORDER = ('view', 'sparsification', 'pseudo_lidar', 'mesh', 'sweep', 'freeview', 'stats', 'components')  # of the products' JSON lines, as they were added


def extra_lines(products):
    """One JSON line {key: summary()} per product that has a summary, with what the product wants beside its key."""
    lines = {p.key: dict({p.key: p.summary()}, **getattr(p, 'beside', {})) for p in products if hasattr(p, 'summary')}
    for key in LINE_ORDER + LATER_LINE_ORDER + GROUND_LINE_ORDER:
        if key in lines:
            print(json.dumps(lines[key]))


def write_tables(save_path, results):
    """view_errors.txt, sparsification.txt and cloud_errors.txt from the products' results, where the run has them."""
    if 'view' in results:
        write_view_errors(os.path.join(save_path, 'view_errors.txt'), results['view'])
    if 'sparsification' in results:
        write_sparsification(os.path.join(save_path, 'sparsification.txt'), results['sparsification'])
    if 'cloud' in results:
        write_cloud_errors(os.path.join(save_path, 'cloud_errors.txt'), results['cloud'])


def main():
    import torch
    from fal_net_amd import inference, synthetic
    from fal_net_amd import myUtils as utils
    import models
    dev = torch.device('cuda', 0)
    dtype = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[args.dtype]
    post = 'flip' if args.f_post_process else ('ms_pp' if args.ms_post_process else 'none')
    refuse_out_of_scope(args)
    check_freeview_fill_args(args)
    check_confidence_args(args)
    check_family_args(args)
    check_component_args(args)
    dataset_mode = bool(args.data) and not args.synthetic
    check_sparsification_args(args, dataset_mode)
    check_cloud_args(args, dataset_mode)
    check_ground_args(args)
    model_dir = checkpoint_path(args)  # :119-120
    have_ckpt = os.path.isfile(model_dir)
    if args.checkpoint and not have_ckpt:
        raise SystemExit('--checkpoint {!r} does not exist'.format(args.checkpoint))
    if dataset_mode and not have_ckpt and not args.allow_seeded_weights:
        raise SystemExit('dataset mode evaluates a trained model, but the checkpoint {!r} does not exist: it is composed as '
                         '<-dt>/<-ts>/<-m><-dtl> (reference Test_KITTI.py:119-121), or give --checkpoint <file.pth.tar>'.format(model_dir))
    if have_ckpt:
        data = torch.load(model_dir, map_location='cpu')
        print("=> using pre-trained model for pan '{}'".format(data.get('m_model', args.model)))
    else:
        data = {'state_dict': synthetic.seeded_state_dict(args.model[-1], args.no_levels)}
    m_name = data.get('m_model', args.model) if isinstance(data, dict) else args.model  # :122
    pan_model = models.__dict__[m_name](data, no_levels=args.no_levels, compute_dtype=dtype).to(dev).eval()
    n_params = utils.get_n_params(pan_model)
    save_path = args.save_path or (os.path.join('Test_Results', args.tdataName, args.model, args.time_stamp)  # :81-85
                                   + ('fpp' if args.f_post_process else '') + ('mspp' if args.ms_post_process else ''))

    def make_products(triples=None):
        """The run's products, in the order every frame goes through them (inference.run_products).  triples: the frames of dataset mode."""
        from fal_net_amd import confidence, dumps, freeview, mesh, pseudo_lidar, views
        from fal_net_amd import sparsification as SP
        n_frames, products = len(triples) if triples else 1, []
        if args.sparsification is not None:
            products.append(SP.SparsificationTable(n_frames, args.sparsification, args.sparsification_steps or SP.DEFAULT_STEPS, dev,
                                                   extra={'file': os.path.join(save_path, 'sparsification.txt')}))
        if args.view_metrics:
            products.append(inference.ViewMetrics(n_frames, dev, beside={'file': os.path.join(save_path, 'view_errors.txt')}))
        if args.dump:
            # with --pc-min-conf the point cloud is the stats writer's: the frame writer keeps the other kinds
            products.append(dumps.FrameWriter(save_path, [k for k in args.dump if k != 'pc' or args.pc_min_conf is None], ply_format=args.ply_format))
        fractions = sweep_fractions(args)
        if fractions is not None:
            try:
                views.check_baselines(fractions)
            except ValueError as e:
                raise SystemExit('--sweep-range: {}'.format(e))
            products.append(dumps.SweepWriter(save_path, fractions, extra={'views': args.sweep, 'range': list(args.sweep_range)}))
        poses = freeview_poses(args)
        if poses is not None:
            try:
                K = freeview.camera(args.height, args.width)
                freeview.check_poses([freeview.pose(K, **kw) for kw in poses])
            except ValueError as e:
                raise SystemExit('--freeview: {}'.format(e))
            extra = {'poses': args.freeview, 'path': args.freeview_path, 'amp': list(args.freeview_amp), 'yaw': args.freeview_yaw, 'camera': 'nominal'}
            if args.freeview_fill is not None:
                from fal_net_amd import inpaint
                extra['fill'] = {'beta': args.freeview_fill, 'floor': inpaint.FLOOR, 'levels': inpaint.levels(args.height, args.width)}
            products.append(freeview.FreeviewWriter(save_path, poses, fill_beta=args.freeview_fill, extra=extra))
        if args.stats is not None or args.pc_min_conf is not None:
            products.append(confidence.StatsWriter(save_path, args.stats or (), pc_min_conf=args.pc_min_conf, ply_format=args.ply_format))
        if args.pseudo_lidar:
            calibration, source = lidar_calibration(args, triples)
            if source == 'nominal':
                print('=> pseudo-LiDAR: no calibration files (--pl-calib, or --velodyne-root on the original split): a nominal camera is used, the '
                      'KITTI focal length and baseline for the image width, the principal point at the image centre, no translation')
            products.append(pseudo_lidar.PseudoLidarWriter(save_path, calibration, beams=args.pl_beams, az_bins=args.pl_az_bins, max_depth=args.pl_max_depth,
                                                           max_height=args.pl_max_height, min_conf=args.pl_min_conf, extra={'calibration': source},
                                                           **({} if args.pl_remove_ground is None else
                                                              {'remove_ground': args.pl_remove_ground, 'ground': ground_fit_args(args)}),
                                                           **({} if args.min_component is None else
                                                              {'min_component': args.min_component,
                                                               'component_jump': 0.05 if args.component_jump is None else args.component_jump})))
        if args.mesh:
            products.append(mesh.MeshWriter(save_path, max_jump=args.mesh_max_jump, max_depth=args.mesh_max_depth, min_conf=args.mesh_min_conf,
                                            normals=args.mesh_normals, ply_format=args.ply_format,
                                            **({} if args.min_component is None else
                                               {'min_component': args.min_component, 'component_jump': args.component_jump})))
        if args.min_component is not None:
            from fal_net_amd import components
            jump = args.component_jump if args.component_jump is not None else (args.mesh_max_jump if args.mesh else 0.05)
            products.append(components.ComponentsSummary(args.min_component, jump))
        if args.cloud_metrics:
            from fal_net_amd import cloud_metrics
            calibration, source = lidar_calibration(args, triples)
            if source == 'nominal':
                print('=> cloud metrics: no calibration files (--pl-calib, or --velodyne-root on the original split): a nominal camera is used, the '
                      'KITTI focal length and baseline for the image width, the principal point at the image centre, no translation')
            products.append(cloud_metrics.CloudMetrics(n_frames, calibration, thresholds=args.cm_thresholds or cloud_metrics.THRESHOLDS, on=args.cm_on,
                                                       beams=args.cm_beams, max_depth=args.cm_max_depth, device=dev,
                                                       beside={'file': os.path.join(save_path, 'cloud_errors.txt'), 'calibration': source}))
        if args.ground:
            from fal_net_amd import ground
            calibration, source = lidar_calibration(args, triples)
            if source == 'nominal':
                print('=> ground: no calibration files (--pl-calib, or --velodyne-root on the original split): a nominal camera is used, the '
                      'KITTI focal length and baseline for the image width, the principal point at the image centre, no translation')
            products.append(ground.GroundPlanes(save_path, calibration, max_depth=args.pl_max_depth, extra={'calibration': source}, **ground_fit_args(args)))
        return products

    if dataset_mode:
        from fal_net_amd import datasets as DS
        args.batch_size = 1  # kitty mixes image sizes! (:112)
        args.sparse = True  # disparities are sparse (from lidar) (:113)
        root = os.path.join(args.data, args.tdataName)
        if args.tdataName == 'Kitti_eigen_test_original':
            triples = DS.eigen_original_triples(resolve_test_list(args), root, args.velodyne_root)
            dataset = DS.StereoEvalDataset(root, triples, cam=args.velodyne_cam)
        else:
            triples = DS.kitti2015_pairs(root) if args.tdataName == 'Kitti2015' else DS.eigen_test_triples(args.test_list, root)
            dataset = DS.StereoValDataset(root, triples)
        if not triples:
            raise SystemExit('no test frame with ground truth found under {}'.format(root))
        loader = DS.make_loader(dataset, 1, args.workers, shuffle=False, drop_last=False)  # B = 1: KITTI mixes sizes (:113)
        os.makedirs(save_path, exist_ok=True)
        with open(os.path.join(save_path, 'settings.txt'), 'w') as f:  # :63-75
            hidden = settings_left_out(args) + ground_left_out(args)
            f.write(''.join('%15s: %s\n' % (k, v) for k, v in vars(args).items() if k not in hidden))
        print('=> {} test frames under {}; saving to {}'.format(len(triples), root, save_path))
        products = make_products(triples)
        res = inference.evaluate(pan_model, loader, data_name=args.tdataName, max_disp=args.max_disp, min_disp=args.min_disp,
                                 rel_baseline=args.rel_baselne, post=post, use_median=args.median, print_freq=args.print_freq,
                                 with_metrics=args.evaluate, device_percentile=args.device_percentile, device_metrics=args.device_metrics,
                                 disparity=args.disparity, products=products)
        write_tables(save_path, res)
        with open(os.path.join(save_path, 'errors.txt'), 'w') as f:  # :277-280
            f.write('\nNumber of parameters {}\n'.format(n_params))
            f.write('\nEPE {}\n'.format(res['epe']))
            f.write('\nKitti metrics: \n{}\n'.format(res['kitti_table']))
        if args.evaluate:  # :282-284
            print('* EPE: {0}'.format(res['epe']))
            print(res['kitti_table'])
        extra_lines(products)
        print(json.dumps({'dataset': args.tdataName, 'frames': res['n'], 'dtype': args.dtype, 'post': post, 'epe': res['epe'], 'kitti': res['kitti'],
                          'sec_per_image': res['sec_per_image'], 'errors_txt': os.path.join(save_path, 'errors.txt')}))
        return

    products = make_products()
    left, _, _, _ = synthetic.synthetic_pair(1, args.height, args.width, seed=7)
    left = left.to(dev)
    max_disp = torch.tensor([args.max_disp * args.rel_baselne], device=dev).view(1, 1, 1)  # Test_KITTI.py:181-182
    min_disp = max_disp * args.min_disp / args.max_disp
    times = []
    with torch.no_grad():
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.time()
            if args.disparity == 'peak':
                disp = inference.peak_disparity(pan_model, left, min_disp, max_disp)
            else:
                disp = pan_model(left, min_disp, max_disp, ret_disp=True, ret_subocc=False, ret_pan=False)  # :196
            if args.f_post_process:
                disp = inference.flip_post_process(left, pan_model, disp, min_disp, max_disp)
            elif args.ms_post_process:
                disp = inference.ms_pp(left, pan_model, disp, min_disp, max_disp, args.device_percentile)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        # the one seeded frame, after the timed loop.  The timed image is seeded noise and its pair's right image is independent of it: no view
        # metric means anything there.  The view is judged on a seeded pair with real geometry instead (synthetic.structured_stereo: the right image
        # IS the left one resampled along a smooth disparity field), at the same size: one more forward on the plan of the timed one
        if args.view_metrics:
            s_left, s_right = synthetic.structured_stereo(1, args.height, args.width, seed=7)[:2]
            inference.run_products([p for p in products if p.key == 'view'],
                                   inference.Frame(0, pan_model, s_left.to(dev), None, min_disp, max_disp, right=s_right.to(dev)))
        inference.run_products([p for p in products if p.key != 'view'], inference.Frame(0, pan_model, left, disp, min_disp, max_disp))
    results = {p.key: p.result() for p in products if hasattr(p, 'result')}
    if results:
        os.makedirs(save_path, exist_ok=True)
    write_tables(save_path, results)
    extra_lines(products)
    print(json.dumps({'image': [args.height, args.width], 'dtype': args.dtype, 'post': post,
                      'sec_per_image_median': sorted(times)[len(times) // 2], 'disp_mean': float(disp.mean()), 'disp_max': float(disp.max())}))


if __name__ == '__main__':
    args = parser.parse_args()
    if args.gpu_no is not None:  # :363, before anything touches the GPU
        os.environ['HIP_VISIBLE_DEVICES'] = str(args.gpu_no)
    main()
