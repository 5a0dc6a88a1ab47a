"""ace_amd -- MI355X-native 2ACE ADMM channel recovery (HIP kernels behind a C-ABI).

Importing this package loads ``libace.so``; it raises if the HIP library has
not been built (there is no CPU fallback on the product path).
"""
from ._lib import LIB, AceError, AdmmCfg, default_cfg  # noqa: F401
from ._lib import (ACE_VARIANT_A2ONLY, ACE_VARIANT_NUCLEAR, ACE_ST_CONVERGED, ACE_ST_NO_OPT,  # noqa: F401
                   ACE_ST_EIG_NOCONV, ACE_ST_ROLLBACK, PipelineCfg, pipeline_cfg)
from .solver import (InferADMM, infer_admm_batch, infer_admm_host, synth_problem, BatchResult,  # noqa: F401
                     nuclear_prox_batch)
from ._lib import path_counts  # noqa: F401
from .pipeline import (inferLowRankV4_multi, inferLowRankV4, inferLowRank_Nuclear,  # noqa: F401
                       infer_low_rank_pipeline_host, infer_low_rank_pipeline_batch, draw_partitions,
                       PipelineResult, SpectralInitialize)
from .phaselift import MyPhaseLift, phaselift_host, phaselift_batch, PhaseLiftResult, prox_eig_host  # noqa: F401
from .beamformer import (svd_beamformer, svd_beamformer_compensation, codebook_beams,  # noqa: F401
                         svd_beamformer_host, svd_beamformer_batch, BeamResult)
from .evaluate import evaluate_host, evaluate_batch, EvalResult  # noqa: F401
from .rss import evaluate_rss_host, evaluate_rss_batch, dbm_to_amp, RssEval  # noqa: F401
from .scan import beam_scan_host, beam_scan_batch, ScanResult  # noqa: F401
from .omp import omp_host, omp_batch, OmpResult  # noqa: F401
from .gamp import embgamp_host, embgamp_batch, GampResult  # noqa: F401
from .prgamp import prgamp_host, prgamp_batch, prgamp_draws, PrGampResult  # noqa: F401
from .minl2 import (minl2_admm_host, minl2_admm_batch, infer_min_l2_host, infer_min_l2_batch, inferMinL2,  # noqa: F401
                    MinL2Stage, MinL2Result)
from ._lib import MinL2Cfg, minl2_cfg  # noqa: F401
from ._lib import ACE_ST_EVAL_DEGENERATE, ACE_ST_OMP_DEPENDENT  # noqa: F401
from ._lib import ACE_ST_GAMP_NANBREAK, ACE_ST_GAMP_MAXEM, ACE_ST_GAMP_FAILED, GampCfg, gamp_cfg  # noqa: F401
from ._lib import ACE_ST_PRGAMP_FAILED, ACE_ST_PRGAMP_MAXTRY, PrGampCfg, prgamp_cfg  # noqa: F401
from . import synth, engine, montecarlo, linops, zprox, realtrace, scan, angular, omp, gamp, prgamp, sparse, minl2  # noqa: F401
from . import stages, nms, pcode, plstep, ustep  # noqa: F401
from .design import aopt_select_batch, aopt_select_host, bayes_beam, AoptResult  # noqa: F401
from ._lib import ACE_ST_AOPT_SINGULAR, AoptCfg, aopt_cfg  # noqa: F401
from . import design  # noqa: F401
from .scenario import scenario_batch, ScenarioResult  # noqa: F401
from ._lib import ScenarioCfg, scenario_cfg  # noqa: F401
from . import scenario  # noqa: F401
from .recovery_eval import (evaluate_recovery_host, evaluate_recovery_batch, recovery_tables, sweep_tables,  # noqa: F401
                            RecoveryEval, RecoveryTables, SweepTables, METRICS_RECOVERY)
from ._lib import ACE_ST_RECEVAL_NOSWEEP  # noqa: F401
from . import recovery_eval  # noqa: F401

__version__ = LIB.ace_version().decode()
