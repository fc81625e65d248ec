"""CLI mirror of ``article_separation/plot_net_output.py``: score a segmentation net against ground truth channel images.

The reference's flags, names and defaults (:287-298).  Its ``__main__`` then ignores most of them and calls
``plot_net_output`` with constants written into the file (a model path, ``fixed_height=1500``, ``plot_with_img=True``,
``mask_threshold=True``, ``show_plot=True``, ``calculate_accuracy=False``); here the flags are honoured, and the function's
remaining keyword arguments are flags of their own with the function's defaults (:131-133).  ``--dtype`` and
``--pages_per_call`` are this project's.  The work is ``seg_eval.plot_net_output``.
"""
import argparse

from . import cli_flags

DTYPES = ("f32", "bf16", "f32s")


def build_parser():
    parser = argparse.ArgumentParser()
    # -- the reference's parser (:287-298)
    parser.add_argument('--path_to_tf_graph', type=str,
                        help="path to the pixel labelling graph (TF1 frozen .pb or .asepw).")
    parser.add_argument('--path_to_img_lst', type=str,
                        help='path to the lst file containing the file paths of the images.')
    parser.add_argument('--save_folder', type=str, help="path to the save folder")
    parser.add_argument('--rescale_factor', default=1.0, type=float,
                        help="rescaling the images before inputting them to the network.")
    parser.add_argument('--fixed_height', default=0, type=int,
                        help="rescales the input images to a fixed height. Only works if rescale_factor is not set")
    parser.add_argument('--calculate_accuracy', default=False, action='store_true',
                        help="whether or not to calculate the accuracy of the net output - needs GT "
                             "(<dir>/C<n>/<name>_GT<i>.png, of the net output's size: other sizes are refused, because the "
                             "reference's OpenCV bilinear resize of them cannot be reproduced here).  Also prints precision, "
                             "recall, F1 and IoU per class, an addition to the reference.")
    # -- keyword arguments of the reference's plot_net_output (:131-133), which its __main__ sets in the file
    parser.add_argument('--mask_threshold', default=None, type=float,
                        help="thresholds the net output before the arg max and the masks.  As in the reference (:201-202) the "
                             "flag only switches thresholding on: the threshold is 0.6 whatever value is given (0 = off).")
    parser.add_argument('--plot_with_gt', default=False, action='store_true',
                        help="write the ground truth to the right of the net output - needs GT.")
    parser.add_argument('--plot_with_img', default=False, action='store_true',
                        help="write the net output blended over the scan instead of the masks alone.")
    parser.add_argument('--show_plot', default=False, action='store_true',
                        help="accepted; plots on the screen (matplotlib) are not part of this build, which says so once.")
    parser.add_argument('--gpu_device', default="0", type=str, help="the device to run on.")
    # -- this project's
    parser.add_argument('--dtype', default=None, choices=DTYPES,
                        help="arithmetic of the net: f32, bf16 or f32s (default: what the model file says).")
    parser.add_argument('--pages_per_call', type=cli_flags.pages_per_call, default=1,
                        help="pages of one forward and one scoring call.")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.path_to_tf_graph or not args.path_to_img_lst:
        raise SystemExit("--path_to_tf_graph and --path_to_img_lst are needed")
    from . import seg_eval
    seg_eval.plot_net_output(args.path_to_tf_graph, args.path_to_img_lst, args.save_folder or "", gpu_device=args.gpu_device,
                             rescale=args.rescale_factor, fixed_height=args.fixed_height, mask_threshold=args.mask_threshold,
                             plot_with_gt=args.plot_with_gt, plot_with_img=args.plot_with_img, show_plot=args.show_plot,
                             calculate_accuracy=args.calculate_accuracy, pages_per_call=args.pages_per_call, dtype=args.dtype)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
