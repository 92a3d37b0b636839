#!/usr/bin/env python3
"""Genie construction of a polar code for a binary memoryless channel as one device pipeline
(coding.genieEncodeDecodeSimulationDeviceBin): BI-AWGN at a given Eb/N0 and rate (or noise
variance), or BSC(p).

    python -m polarcub_amd.cli.genie_bin --channel awgn --ebn0 2 --rate 0.5 -n 10 -g 1000000 -e 0.1 -f frozen.txt

The trials are drawn on the device from the genie seed (Philox streams keyed by the seed and the
trial index).  The file is the reference's frozen-bits format: coding.read_frozen_file (the reader
of main_deletion) reads it back and encodeDecodeSimulation takes the set.
"""
import argparse

from .. import coding, construction, mc


def parser():
    ap = argparse.ArgumentParser(description="genie construction for a binary memoryless channel on the GPU")
    ap.add_argument("--channel", choices=("awgn", "bsc"), default="awgn", help="The channel. Default is awgn.")
    ap.add_argument("--ebn0", type=float, help="BI-AWGN: Eb/N0 in dB (with --rate).")
    ap.add_argument("--rate", type=float, default=0.5, help="BI-AWGN: the code rate Eb/N0 refers to. Default is 0.5.")
    ap.add_argument("--sigma2", type=float, help="BI-AWGN: the noise variance, instead of --ebn0 / --rate.")
    ap.add_argument("-p", "--crossover-probability", type=float, default=0.11,
                    help="BSC: the crossover probability. Default is 0.11.")
    ap.add_argument("-n", "--n", type=int, required=True, help="The number of polarization steps.")
    ap.add_argument("-g", "--genie-simulations", type=int, default=8000, help="Genie trials. Default is 8000.")
    ap.add_argument("-e", "--error-probability", type=float, default=0.1,
                    help="Upper bound on error probability, when constructing the frozen set. Default is 0.1.")
    ap.add_argument("-gs", "--genie-seed", type=int, default=300, help="Seed of the genie's trials. Default is 300.")
    ap.add_argument("-f", "--frozen-bits-file", help="Write the frozen bits to a file.")
    return ap


def channel_of(args):
    """(mc channel code, its parameter) of the parsed arguments."""
    if args["channel"] == "bsc":
        p = args["crossover_probability"]
        if not 0.0 <= p <= 1.0:
            raise ValueError("the crossover probability must be in [0, 1]")
        return mc.CHANNEL_BSC, p
    if args["sigma2"] is not None:
        if args["ebn0"] is not None:
            raise ValueError("give --sigma2 or --ebn0 / --rate, not both")
        sigma2 = args["sigma2"]
    elif args["ebn0"] is not None:
        if not 0.0 < args["rate"] <= 1.0:
            raise ValueError("the rate must be in (0, 1]")
        sigma2 = construction.awgn_sigma2(args["ebn0"], args["rate"])
    else:
        raise ValueError("the BI-AWGN channel needs --ebn0 (with --rate) or --sigma2")
    if not sigma2 > 0.0:
        raise ValueError("the noise variance must be positive")
    return mc.CHANNEL_AWGN, sigma2


def main(argv=None):
    args = vars(parser().parse_args(argv))
    channel, param = channel_of(args)
    n, G, bound = args["n"], args["genie_simulations"], args["error_probability"]
    filename = args["frozen_bits_file"]
    print("n =", n, ", channel =", args["channel"], ", parameter =", param)
    if filename is not None:
        print("frozen bits file = ", filename)
    print("performing", G, "genie encoding/decoding trials to find a frozen set with WER at most", bound)
    return coding.genieEncodeDecodeSimulationDeviceBin(n, channel, param, G, bound, args["genie_seed"],
                                                       filename=filename)


if __name__ == "__main__":
    main()
