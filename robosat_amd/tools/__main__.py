"""``rs`` entry point for the hot-path tools and their immediate callers: ``rs train``,
``rs predict``, ``rs weights``, ``rs masks``, ``rs features``, ``rs evaluate``, ``rs serve``.  The reference's
``robosat/tools/__main__.py`` registers 15 tools; the other 9 are dataset preparation / vector post-processing and out of scope here
(``rs evaluate`` covers what its ``rs compare --minimum/--maximum`` is used for: ranking tiles by how wrong the model is)."""

import argparse

from robosat_amd.tools import evaluate, features, masks, predict, serve, train, weights


def add_parsers():
    parser = argparse.ArgumentParser(prog="./rs")
    subparser = parser.add_subparsers(title="robosat tools", metavar="")
    train.add_parser(subparser)
    predict.add_parser(subparser)
    weights.add_parser(subparser)
    masks.add_parser(subparser)
    features.add_parser(subparser)
    evaluate.add_parser(subparser)
    serve.add_parser(subparser)
    subparser.required = True
    return parser.parse_args()


def main():
    args = add_parsers()
    args.func(args)


if __name__ == "__main__":
    main()
