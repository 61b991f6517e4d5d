"""python -m xrnerf_amd.run_nerf --config CONFIG --dataname NAME [--test_only] [--render_only] [--load_from FILE]: the reference's
run_nerf.py (train, or test with --test_only) over a reference config file, through xrnerf_amd.apis"""
from .apis import parse_args, run_nerf


def main(argv=None):
    run_nerf(parse_args(argv))


if __name__ == '__main__':
    main()
