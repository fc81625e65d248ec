"""Command-line grammar of the reference's flag system (``python_util/basic/flags.py``), restated on argparse:

  * ``@path/to/config`` files whose lines hold ``--flag value ...``, ``=`` separators and ``#`` comments (flags.py:10-28);
  * dict flags ``--input_params k=v k2=[a,b]`` with automatic typing: true/t/false/f -> bool, numbers -> int when integral
    else float, ``[..]`` -> list of typed elements, everything else stays a string (flags.py:228-285);
  * ``update_params``: unknown keys are reported with ``logging.critical`` but still merged (flags.py:303-333).

Pinned by golden vectors captured from the imported reference (tests/golden/make_flags_golden.py).
"""
import argparse
import logging


class LineArgumentParser(argparse.ArgumentParser):
    def convert_arg_line_to_args(self, arg_line):
        args = arg_line.split()
        for i, arg in enumerate(args):
            if arg == "#":
                return args[:i]
            if arg == "=":
                args.remove("=")
        return args


def _typed(s):
    low = s.lower()
    if low in ("true", "t"):
        return True
    if low in ("false", "f"):
        return False
    try:
        f = float(s)
    except ValueError:
        return s
    i = int(f)
    return i if i == f else f


def parse_key_value(kv_list, into=None):
    """The body of StoreDictKeyPair.__call__ (flags.py:252-285)."""
    out = {} if into is None else into
    for kv in kv_list:
        parts = kv.split("=")
        if len(parts) != 2:
            continue
        key, val = parts
        s = val.strip()
        typed = _typed(val)
        if isinstance(typed, str) and len(s) >= 1 and s[0] == "[" and s[-1] == "]":
            elems = [e.strip() for e in s[1:-1].split(",")]
            typed = [_typed(e) for e in elems if e != ""]
        out[key] = typed
    return out


class StoreDictKeyPair(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        if not getattr(namespace, self.dest):
            setattr(namespace, self.dest, {})
        parse_key_value(values, getattr(namespace, self.dest))


def parse_feature_map_layout(kv_list):
    """``--feature_map_generation_params from_layer=[a,,] layer_depth=[-1,32,32]`` as feature_map_generators.py:95-97 prescribes it
    (no spaces, no quotes) -> (from_layer or None, layer_depth or None).  Unlike the generic dict flag, which drops empty list elements
    (flags.py:281-282), the EMPTY from_layer entries are kept: they are the layout's "new map from the previous one".  The keys the
    engine does not build are refused with the reason; other keys (layer_compressed_dim ...) belong to the export and are ignored here."""
    layers = depths = None
    for kv in kv_list or ():
        parts = kv.split("=")
        if len(parts) != 2:
            continue
        key, val = parts[0].strip(), parts[1].strip()
        is_list = len(val) >= 2 and val[0] == "[" and val[-1] == "]"
        elems = [e.strip() for e in val[1:-1].split(",")] if is_list else [val]
        if key in ("use_depthwise", "use_explicit_padding"):
            if _typed(val) is not False:
                raise ValueError(f"feature_map_generation_params {key}={val}: only the plain SAME-padded 3x3 convolution is built "
                                 "(depthwise and explicitly padded variants are not served)")
        elif key == "conv_kernel_size":
            if any(_typed(e) not in (3, -1) for e in elems if e != ""):
                raise ValueError(f"feature_map_generation_params conv_kernel_size={val}: generated maps use the 3x3 convolution "
                                 "(-1 for the plain from_layer entries); other kernel sizes are not served")
        elif key == "from_layer":
            if not is_list:
                raise ValueError(f"feature_map_generation_params from_layer={val}: a list [name,name,,] is expected")
            layers = [] if val[1:-1].strip() == "" and "," not in val else [str(e) for e in elems]
        elif key == "layer_depth":
            try:
                depths = [int(e) for e in elems if e != ""]
            except ValueError:
                raise ValueError(f"feature_map_generation_params layer_depth={val}: a list of whole numbers is expected")
    return layers, depths


class StoreFeatureMapLayout(StoreDictKeyPair):
    """the dict flag as the reference parses it, plus ``<dest>_layout`` = parse_feature_map_layout of the same tokens"""
    def __call__(self, parser, namespace, values, option_string=None):
        super().__call__(parser, namespace, values, option_string)
        try:
            setattr(namespace, self.dest + "_layout", parse_feature_map_layout(values))
        except ValueError as e:
            parser.error(str(e))


def define_feature_map_layout(parser, default=None):
    """--feature_map_generation_params (the reference's spelling) and --visual_layers / --visual_layer_depths (this project's)"""
    parser.add_argument("--feature_map_generation_params", action=StoreFeatureMapLayout, default={} if default is None else default, nargs="*",
                        metavar="KEY=VAL")
    parser.set_defaults(feature_map_generation_params_layout=(None, None))
    parser.add_argument("--visual_layers", type=str, nargs="*", default=None)
    parser.add_argument("--visual_layer_depths", type=int, nargs="*", default=None)


def visual_layout(flags):
    """(visual_layers or None, visual_layer_depths or None) of parsed flags: either spelling, ``ValueError`` if both are given and differ"""
    fl, ld = getattr(flags, "feature_map_generation_params_layout", (None, None))
    vl, vd = getattr(flags, "visual_layers", None) or None, getattr(flags, "visual_layer_depths", None) or None
    if fl is not None and vl is not None and list(fl) != list(vl):
        raise ValueError(f"--visual_layers {vl} and --feature_map_generation_params from_layer={fl} differ")
    if ld is not None and vd is not None and list(ld) != list(vd):
        raise ValueError(f"--visual_layer_depths {vd} and --feature_map_generation_params layer_depth={ld} differ")
    layers = vl if vl is not None else fl
    depths = vd if vd is not None else ld
    if depths is not None and all(d == -1 for d in depths) and (layers is None or len(layers) == len(depths)):
        depths = None                                        # the default layout
    return (list(layers) if layers is not None else None), (list(depths) if depths is not None else None)


def define_dict(parser, name, default, doc=""):
    parser.add_argument("--" + name, action=StoreDictKeyPair, default=default, nargs="*", metavar="KEY=VAL", help=doc)


def str2bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() in ("true", "t", "1")


def update_params(class_params, flag_params, name=""):
    for k in flag_params:
        if k not in class_params:
            logging.critical("Given {0}_params-key '{1}' is not used by {0}-class!".format(name, k))
    class_params.update(flag_params)
    return class_params


def pages_per_call(text):
    """argparse type of ``--pages_per_call`` (run_gnn_clustering, lav_rel): pages of one engine call, at least 1 (= page by page)"""
    try:
        n = int(text)
    except (TypeError, ValueError):
        raise argparse.ArgumentTypeError(f"--pages_per_call takes a whole number of pages, got {text!r}")
    if n < 1:
        raise argparse.ArgumentTypeError(f"--pages_per_call {n}: a call takes at least one page (1 = page by page, the default)")
    return n
